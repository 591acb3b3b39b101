"""The hogwild VEBPR step cases (tests/vebpr_step_cases.py) are fair tests, their tolerances follow their rules, and their
checks are sharp — all from the CPU restatement of the sampler and the float64 step, without a device."""
import numpy as np
import pytest

import vebpr_step_cases as vc
from oracle import vebpr_step_oracle as step


def _as_device(tables64):
    """what a device holding float32 tables would return for these float64 results"""
    return tuple(np.asarray(t, np.float32) for t in tables64)


def _c_measured(c):
    """largest |sequential - jacobi| / path over the touched rows of both tables, three orders of application"""
    n = len(c.quad[0])
    rs = np.random.RandomState(len(c.name) + c.k)
    worst = 0.0
    for order in (np.arange(n), rs.permutation(n), rs.permutation(n)):
        seq = step.sequential(c.quad, c.tables, vc.LR_B, vc.REG, vc.ALPHA, order)
        for tab, start, s in zip("UV", c.tables, seq):
            j = c.jac[tab]
            rows = np.flatnonzero(j["touches"] > 0)
            dev = np.linalg.norm(s[rows] - start[rows].astype(np.float64) - j["sum"][rows], axis=1)
            worst = max(worst, float((dev / j["path"][rows]).max()))
    return worst


_T32 = {}  # per case, filled as the cases go by


def _t32_measured(c):
    """largest |float32 step - float64 step| over the clean rows"""
    if c.name in _T32:
        return _T32[c.name]
    cq = tuple(a[c.clean] for a in c.quad)
    view = cq[2] >= 0
    _, nu, nvi, nvv, nvj = step.step_f32(cq, c.tables, vc.LR_A, vc.REG, vc.ALPHA)
    got = {"U": nu, "V": np.concatenate([nvi, nvj, nvv[view]])}
    errs = [np.abs(got[tab] - c.clean_want[tab]) for tab in "UV"]
    _T32[c.name] = max([float(e.max()) for e in errs if e.size] + [0.0])
    return _T32[c.name]


@pytest.mark.parametrize("name", vc.NAMES)
def test_case_is_a_fair_test_and_its_tolerances_follow_their_rules(oracle, name):
    c = vc.case(name)
    u, i, v, j = c.quad
    n_quad = len(u)
    # a whole epoch: nnz draws (owned: the sum of the slices, which is nnz again)
    assert c.draws == n_quad + c.skipped == c.nnz
    assert c.skipped == c.skipped_purchase + c.skipped_view_only
    if c.form == "owned":
        assert c.draws == int(np.diff(c.own_tables[0]).sum())
        assert vc.ownership_applies(c.nnz, vc.MI355X_CUS)
    elif c.data == "small":
        assert not vc.ownership_applies(c.nnz, vc.MI355X_CUS // 4), "far below the ownership threshold: the dispatcher picks the unowned kernels"
    for start in c.tables:
        assert start.dtype == np.float32
    # real scores: z well away from 0.5 on both sides
    z = 1.0 / (1.0 + np.exp(c.x[c.applies]))
    z05, z95 = np.quantile(z, [0.05, 0.95])
    assert z05 <= 0.25 and z95 >= 0.75, (z05, z95)
    ambiguous = int(((np.abs(c.x) < c.x_bound) & c.applies).any(axis=1).sum())
    assert ambiguous <= max(2, n_quad // 10_000), "the float32 score bound decides nearly every sign: %d of %d ambiguous" % (ambiguous, n_quad)
    lo, hi = vc.correct_interval(c)
    assert hi - lo <= ambiguous
    # launch A: enough clean quadruples of both kinds; the skips and the v == i rows that the data was built for
    clean_view, clean_plain = int((c.clean & c.has_v).sum()), int((c.clean & ~c.has_v).sum())
    v_is_i = int((v == i).sum())
    if c.data == "small":
        assert clean_view >= 300 and clean_plain >= 300, (clean_view, clean_plain)
        assert c.skipped_purchase >= 50 and c.skipped_view_only >= 50, (c.skipped_purchase, c.skipped_view_only)
        assert v_is_i >= 30, v_is_i
    tu, tv = c.touches["U"], c.touches["V"]
    if c.data == "large":
        assert tu[tu > 0].mean() < 5 and tv[tv > 0].mean() < 5, "few touches per row"
    if c.form == "owned":
        assert c.shared.any() and not c.shared.all(), "exclusive users (plain stores) and shared ones (atomics) both occur"
        # every wave's last tile is partial (the mask of the owned form's last tile)
        lens = np.diff(c.own_tables[0])
        assert (lens % 64 != 0).mean() > 0.9 and (lens > 64).mean() > 0.9, "slices of more than one tile, the last one partial"
    if name == "unowned_stride_k64":
        assert -(-c.nnz // 64) > vc.vebpr_grid_waves(vc.MI355X_CUS), "more tiles than waves: some waves loop twice"
    # rows beyond the trained range and untouched rows exist, so "bit-identical" is a real check
    assert (tv[c.ni:] == 0).all() and len(tv) - c.ni == vc.PAD_ROWS and (tv[:c.ni] == 0).any() and (tu == 0).any()
    # T_CLEAN covers the float32 step with its 4x margin
    t32 = _t32_measured(c)
    assert c.no_a or t32 <= vc.T_CLEAN / 4, (t32, vc.T_CLEAN)
    # C[case]: 4 x measured, rounded up to one significant digit
    cm = _c_measured(c)
    vis = {tab: vc.visibility(c, tab) for tab in "UV"}
    print("\n%s: %d quadruples (%d with a view, %d with v == i; skipped: %d by the purchase row, %d by the view row only), clean: "
          "%d with a view, %d without, z 5..95 %% = %.2f..%.2f, %d ambiguous signs, touches max U %d V %d, mean U %.2f V %.2f, "
          "%d untouched item rows, float32 step error %.3g, c measured %.3g -> C = %.3g, single-update visibility %s%s" % (
              name, n_quad, int(c.has_v.sum()), v_is_i, c.skipped_purchase, c.skipped_view_only, clean_view, clean_plain, z05, z95,
              ambiguous, tu.max(), tv.max(), tu[tu > 0].mean(), tv[tv > 0].mean(), int((tv[:c.ni] == 0).sum()), t32, cm,
              vc.round_up_1sig(4 * cm), ", ".join("%s %.2f" % kv for kv in vis.items()),
              "" if c.shared is None else ", %d quadruples of shared users" % int(c.shared.sum())))
    assert 4 * cm <= vc.C[name] <= vc.round_up_1sig(4 * cm * 1.05), (name, cm, vc.round_up_1sig(4 * cm))
    # launch B: one lost or doubled update shows on at least half of the touched rows
    if name != "unowned_stride_k64":
        assert min(vis.values()) >= 0.5, vis


def test_t_clean_follows_its_rule(oracle):
    names = [name for name in vc.NAMES if not vc.SPECS[name].get("no_a")]
    worst = max(_T32[name] if name in _T32 else _t32_measured(vc.case(name)) for name in names)
    print("\nfloat32 step vs float64 step over the clean rows of all cases: %.3g -> T_CLEAN = %.3g" % (worst, vc.round_up_1sig(4 * worst)))
    assert vc.T_CLEAN == vc.round_up_1sig(4 * worst)


# ---- the checks are sharp: a reference with each fault the suite could not see before must fail A or B -------------------
MUTANTS = list(step.FAULTS) + ["row_written_to_the_wrong_item", "one_update_lost", "one_update_doubled"]


def _fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


@pytest.fixture(scope="module")
def mutation_case(oracle):
    c = vc.case("unowned_k7")  # k = 7: a lane group of 8 with one lane beyond k
    good = {lr: step.sequential(c.quad, c.tables, lr, vc.REG, vc.ALPHA) for lr in (vc.LR_A, vc.LR_B)}
    return c, good


def test_the_unmutated_reference_passes_every_check(mutation_case):
    c, good = mutation_case
    vc.check_z(c, c.tables, int(((c.x > 0) | ~c.applies).all(axis=1).sum()), c.skipped)
    worst_a = vc.check_a(c, _as_device(good[vc.LR_A]))
    worst_b = vc.check_b(c, _as_device(good[vc.LR_B]))
    # the Jacobi sums (C) against the per-quadruple deltas (numpy): two statements of the same update
    u, i, v, j = c.quad
    x, dU, dVi, dVv, dVj = step.deltas(c.quad, *c.tables, vc.LR_B, vc.REG, vc.ALPHA)
    want_u, want_v = np.zeros(c.tables[0].shape), np.zeros(c.tables[1].shape)
    np.add.at(want_u, u, dU)
    np.add.at(want_v, np.concatenate([i, j, v[c.has_v]]), np.concatenate([dVi, dVj, dVv[c.has_v]]))
    assert np.abs(want_u - c.jac["U"]["sum"]).max() <= 1e-15 and np.abs(want_v - c.jac["V"]["sum"]).max() <= 1e-15
    assert np.abs(x - c.x).max() <= 1e-13
    # a row with v == i carries both deltas and two touches
    row = int(i[np.flatnonzero(v == i)[0]])
    assert c.touches["V"][row] >= 2
    print("\nsequential float64 reference rounded to float32: A %s, B (error / tolerance) %s" % (worst_a, worst_b))


@pytest.mark.parametrize("mutant", MUTANTS)
def test_checks_reject_a_wrong_update(mutation_case, mutant):
    c, good = mutation_case
    out = {}
    for launch, lr in (("A", vc.LR_A), ("B", vc.LR_B)):
        if mutant in step.FAULTS:
            got = step.sequential(c.quad, c.tables, lr, vc.REG, vc.ALPHA, fault=mutant)
        elif mutant == "row_written_to_the_wrong_item":
            got = tuple(t.copy() for t in good[lr])
            a, b = c.quad[1][np.flatnonzero(c.clean)[:2]]  # two touched item rows change places on the way back
            got[1][[a, b]] = got[1][[b, a]]
        else:
            # a row touched three times by three quadruples, so not a clean one
            u, i, v, j = c.quad
            cand = np.flatnonzero(c.touches["V"] == 3)
            row = int(next(r for r in cand if len(c.quadruples_of("V", r)) == 3))
            got = step.sequential(c.quad, c.tables, lr, vc.REG, vc.ALPHA, **{"drop" if mutant == "one_update_lost" else "double": ("V", row)})
        check = vc.check_a if launch == "A" else vc.check_b
        out[launch] = _fails(check, c, _as_device(got))
    print("\n%s: rejected by %s" % (mutant, " and ".join(k for k, v in out.items() if v) or "NOTHING"))
    assert out["A"] or out["B"], mutant
    if mutant.startswith("one_update"):
        assert out["B"], "only launch B looks at rows touched more than once"
