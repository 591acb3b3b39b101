"""The HPF checks' reference, inputs and tolerances, in ONE place: tests/test_hpf_cpu.py holds the restatement below against
the golden that the reference's own compiled extension wrote (tests/golden/make_hpf_golden.py), tests/test_hpf_gpu.py holds
the device against the restatement and against the same golden.

`hpf_fit` restates hpf_cpp / pf_cpp (cornac/models/hpf/cpp/cpp_hpf.cpp:208-275 / :139-203) in float64 NumPy with
scipy.special.digamma.  K_r = T_r = 1 at the start of the call (hpf.pyx:148-149); hierarchical: computed from the tables
before the loop (cpp_hpf.cpp:231-234).  One iteration, in the reference's order:
  1. Lt = exp(digamma(G_s) - log G_r), Lb = exp(digamma(L_s) - log L_r) — both shape updates below use these two;
  2. G_s[u,f] = 0.3 + sum over u's ratings of Lt[u,f] Lb[i,f] x / dk,  dk = 2^-52 + sum_f Lt[u,f] Lb[i,f];
  3. G_r[u,f] = k_s / K_r[u] + sum_j L_s[j,f] / L_r[j,f] — the L of the iteration BEFORE;
  4. hierarchical: K_r[u] = 0.3 + sum_f G_s[u,f] / G_r[u,f];
  5. L_s[i,f] = 0.3 + the terms of step 2 by item;
  6. L_r[i,f] = t_s / T_r[i] + sum_u G_s[u,f] / G_r[u,f] — the NEW G;
  7. hierarchical: T_r likewise.
k_s = t_s = 0.3 + k 0.3 hierarchical, 0.3 otherwise.  With strictly positive finite tables the reference's detour through
pruned sparse matrices (cpp_hpf.cpp:102-123) is this dense formula.  The sums run in NumPy's order, not the reference's
(which walks the ratings column by column), and digamma / log / exp are other implementations than Eigen's and libm's: the
restatement agrees with the reference to a tolerance, measured per golden case and recorded below.
"""
import functools

import numpy as np

import nmf_cases as nc

F32 = np.float32
F64 = np.float64
PRIOR = 0.3
EPS = 2.0 ** -52


def hpf_fit(rid, cid, val, G_s, G_r, L_s, L_r, n_iters, hierarchical):
    """n_iters iterations from copies of the tables -> (G_s, G_r, L_s, L_r, K_r, T_r)"""
    from scipy.special import digamma

    G_s, G_r, L_s, L_r = (np.array(t, F64, order="C") for t in (G_s, G_r, L_s, L_r))
    rid, cid = np.asarray(rid, np.int64), np.asarray(cid, np.int64)
    assert np.asarray(val).dtype == F32
    x = np.asarray(val).astype(F64)[:, None]
    k = G_s.shape[1]
    k_s = t_s = PRIOR + k * PRIOR if hierarchical else PRIOR
    K_r, T_r = np.ones(G_s.shape[0]), np.ones(L_s.shape[0])
    if hierarchical:
        K_r = PRIOR + (G_s / G_r).sum(axis=1)
        T_r = PRIOR + (L_s / L_r).sum(axis=1)
    with np.errstate(under="ignore"):
        for _ in range(n_iters):
            Lt = np.exp(digamma(G_s) - np.log(G_r))                                  # 1
            Lb = np.exp(digamma(L_s) - np.log(L_r))
            P = Lt[rid] * Lb[cid]
            terms = P * x / (EPS + P.sum(axis=1))[:, None]
            G_s = np.full_like(G_s, PRIOR)                                           # 2
            np.add.at(G_s, rid, terms)
            G_r = k_s / K_r[:, None] + (L_s / L_r).sum(axis=0)[None, :]              # 3: the old L
            if hierarchical:
                K_r = PRIOR + (G_s / G_r).sum(axis=1)                                # 4
            L_s = np.full_like(L_s, PRIOR)                                           # 5
            np.add.at(L_s, cid, terms)
            L_r = t_s / T_r[:, None] + (G_s / G_r).sum(axis=0)[None, :]              # 6: the new G
            if hierarchical:
                T_r = PRIOR + (L_s / L_r).sum(axis=1)                                # 7
    return G_s, G_r, L_s, L_r, K_r, T_r


def elog(S, R):
    """step 1 alone"""
    from scipy.special import digamma

    with np.errstate(under="ignore"):
        return np.exp(digamma(np.asarray(S, F64)) - np.log(np.asarray(R, F64)))


# ---- inputs ------------------------------------------------------------------------------------------------------------
def draw_tables(nu, ni, k, hierarchical, rng):
    """hpf.pyx:118-146 / :51-79: G_s, G_r, L_s, L_r in this order from one generator, gamma(100, 0.003) hierarchical or
    gamma(0.3, 1 / 0.3), cast to float32, reshaped, promoted to double"""
    shape, scale = (100., 0.3 / 100.) if hierarchical else (0.3, 1 / 0.3)
    return tuple(rng.gamma(shape, scale, rows * k).astype(F32).reshape(rows, k).astype(F64) for rows in (nu, nu, ni, ni))


@functools.lru_cache(maxsize=None)
def _case(kind, k, hierarchical):
    src = {"base": lambda: nc.base_case(k), "wide": lambda: nc.wide_case(k), "long": lambda: nc.long_rows_case(k),
           "small": lambda: nc.random_case(60, 40, 600, k, seed=9)}[kind]()
    tables = draw_tables(src["nu"], src["ni"], k, hierarchical, np.random.RandomState(77 + k + 1000 * int(hierarchical)))
    for t in tables:
        t.setflags(write=False)
    assert all((t > 0).all() and np.isfinite(t).all() for t in tables)
    return dict(rid=src["rid"], cid=src["cid"], val=src["val"], nu=src["nu"], ni=src["ni"], k=k, hierarchical=hierarchical,
                tables=tables)


def base_case(k=5, hierarchical=True):
    """48 users x 32 items x 256 ratings (the cells of nmf_cases.base_case) with the variant's start tables"""
    return _case("base", k, bool(hierarchical))


def wide_case(k=15, hierarchical=True):
    """300 users x 200 items x 5000 ratings (the cells of nmf_cases.wide_case)"""
    return _case("wide", k, bool(hierarchical))


def small_case(k=5, hierarchical=True):
    """60 users x 40 items x 600 ratings (the cells of the NMF golden's random_case)"""
    return _case("small", k, bool(hierarchical))


def long_rows_case(k=5, hierarchical=True):
    """the cells of nmf_cases.long_rows_case: 1200 users x 200 items x 6000 ratings; item 3 has 1000 raters (at least four
    segments of the split plan), user 0 rates 199 items, user 1199 one, user 7 and item 11 none — their shapes must come out
    as exactly the prior"""
    return _case("long", k, bool(hierarchical))


def run_restatement(case, n_iters):
    return hpf_fit(case["rid"], case["cid"], case["val"], *case["tables"], n_iters, case["hierarchical"])


# the golden file's given-tables cases: name -> (case maker, k, iterations)
GOLDEN_GIVEN = {
    "hier_small": (small_case, 5, 5, True), "pf_small": (small_case, 5, 5, False),
    "hier_wide": (wide_case, 15, 3, True), "pf_wide": (wide_case, 15, 3, False),
}
# the seeded cases (init_params all None): name -> (k, iterations, seed, hierarchical); cells of small_case, where every user
# and every item has a rating
GOLDEN_SEEDED = {"hier_seeded": (5, 5, 123, True), "pf_seeded": (5, 5, 123, False)}


def max_rel_diff(got, want):
    """max over the tables of max |got - want| / |want| (want != 0 everywhere: the tables are strictly positive)"""
    worst = 0.0
    for g, w in zip(got, want):
        g, w = np.asarray(g, F64), np.asarray(w, F64)
        assert g.shape == w.shape and (w != 0).all()
        worst = max(worst, float(np.max(np.abs(g - w) / np.abs(w))))
    return worst


# ---- tolerances ----------------------------------------------------------------------------------------------------------
# max relative difference, over the four tables, between the restatement and the reference's compiled extension on each
# golden case (tests/test_hpf_cpu.py measures, prints and holds each to at most this; all must stay below CEILING).  The
# "/it1" entries are the same inputs after ONE iteration.
CEILING = 1e-10
RESTATEMENT_VS_REFERENCE = {
    "hier_small": 1.02e-14, "pf_small": 6.41e-15, "hier_wide": 5.08e-15, "pf_wide": 4.72e-15,
    "hier_small/it1": 2.41e-15, "pf_small/it1": 2.45e-15, "hier_wide/it1": 3.41e-15, "pf_wide/it1": 3.54e-15,
}
DEVICE_FACTOR = 16   # the device differs from the restatement in the ways the restatement differs from the reference
# what tests/test_hpf_gpu.py measured on an MI355X against these tolerances (printed by every run, asserted against the
# tolerances above, not against these): device vs reference on the golden cases, and the worst one-iteration difference
# to the restatement per variant (hierarchical: long rows at k = 40; PF: long rows at k = 5)
DEVICE_VS_REFERENCE_MEASURED = {"hier_small": 3.63e-15, "pf_small": 3.31e-15, "hier_wide": 3.87e-15, "pf_wide": 4.38e-15}
DEVICE_ONE_ITERATION_MEASURED = {"hier": 3.20e-15, "pf": 1.19e-14}


def device_tolerance(name):
    """16 x the case's recorded restatement-against-reference difference, never above the ceiling"""
    return min(DEVICE_FACTOR * RESTATEMENT_VS_REFERENCE[name], CEILING)


def one_iteration_tolerance(hierarchical):
    """for one iteration from the start tables: 16 x the largest one-iteration difference recorded for the variant"""
    pre = "hier_" if hierarchical else "pf_"
    return min(DEVICE_FACTOR * max(v for n, v in RESTATEMENT_VS_REFERENCE.items() if n.startswith(pre) and n.endswith("/it1")),
               CEILING)
