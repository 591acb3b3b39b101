"""The hogwild BPR step cases (tests/bpr_step_cases.py) are fair tests, their tolerances follow their rules, and their
checks are sharp — all from the CPU restatements of the samplers and the float64 step, without a device."""
import numpy as np
import pytest

import bpr_step_cases as bc
from oracle import bpr_step_oracle as step


def _as_device(tables64):
    """what a device holding float32 tables would return for these float64 results"""
    return tuple(np.asarray(t, np.float32) for t in tables64)


def _c_measured(c):
    """largest |sequential - jacobi| / path over the touched rows of all tables, three orders of application"""
    n = len(c.trip[0])
    rs = np.random.RandomState(len(c.name))
    worst = 0.0
    for order in (np.arange(n), rs.permutation(n), rs.permutation(n)):
        seq = step.sequential(c.trip, c.tables, bc.LR_B, bc.REG, c.use_bias, order)
        for tab, start, s in zip("UVB", c.tables, seq):
            j = c.jac[tab]
            rows = np.flatnonzero(j["touches"] > 0)
            if len(rows):
                dev = np.linalg.norm((s[rows] - start[rows].astype(np.float64) - j["sum"][rows]).reshape(len(rows), -1), axis=1)
                worst = max(worst, float((dev / j["path"][rows]).max()))
    return worst


_T32 = {}  # per case, filled as the cases go by


def _t32_measured(c):
    """largest |float32 step - float64 step| over the clean rows"""
    if c.name in _T32:
        return _T32[c.name]
    trip = tuple(a[c.clean] for a in c.trip)
    _, nu, nvi, nvj, nbi, nbj = step.step_f32(trip, c.tables, bc.LR_A, bc.REG, c.use_bias)
    got = {"U": nu, "V": np.concatenate([nvi, nvj]), "B": np.concatenate([nbi, nbj])}
    errs = [np.abs(got[tab] - c.clean_want[tab]) for tab in "UVB"]
    _T32[c.name] = max([float(e.max()) for e in errs if e.size] + [0.0])
    return _T32[c.name]


@pytest.mark.parametrize("name", bc.NAMES)
def test_case_is_a_fair_test_and_its_tolerances_follow_their_rules(oracle, name):
    c = bc.case(name)
    n_trip = len(c.trip[0])
    draws = n_trip + c.skipped
    if c.form == "fused":
        assert draws == c.n
    elif c.form == "ldsbin":  # every bin rounds its share of the launch down at both ends
        assert abs(draws - c.n) < c.plan["bins"]
    else:  # one 64-sample tile of every wave's slice
        assert draws == np.minimum(np.diff(c.ownership[0]), 64).sum()
    for start in c.tables:
        assert start.dtype == np.float32
    # real scores: z well away from 0.5 on both sides
    z = c.z
    z05, z95 = np.quantile(z, [0.05, 0.95])
    assert z05 <= 0.25 and z95 >= 0.75, (z05, z95)
    ambiguous = int((np.abs(c.x) < c.x_bound).sum())
    assert ambiguous <= max(2, n_trip // 10_000), "the float32 score bound decides nearly every sign: %d of %d ambiguous" % (ambiguous, n_trip)
    # launch A: enough clean triplets (LDS bins: enough of them with a hot positive)
    n_clean = int(c.clean.sum())
    n_hot_clean = int((c.clean & c.hot).sum()) if c.hot is not None else None
    if c.clean_share:
        assert n_clean >= 300 and 3 * n_clean >= n_trip, (n_clean, n_trip)
        if c.form == "ldsbin":
            assert n_hot_clean >= 50, n_hot_clean
    elif not c.only_b:
        assert n_clean >= 300, n_clean  # (what exists is still checked: see the case's comment)
    if c.name == "lds_wide_k64":
        assert np.bincount(c.bin, minlength=c.plan["bins"]).min() >= 8 * 16 * 64, "every bin takes the 64-draw tiles"
    # rows beyond the trained range and untouched rows exist, so "bit-identical" is a real check
    tv = c.touches["V"]
    assert (tv[c.ni:] == 0).all() and ((tv[:c.ni] == 0).any() or c.only_b) and tv.max() >= 3
    # T_CLEAN covers the float32 step with its 4x margin
    t32 = _t32_measured(c)
    assert t32 <= bc.T_CLEAN / 4, (t32, bc.T_CLEAN)
    # C[case]: 4 x measured, rounded up to one significant digit
    cm = _c_measured(c)
    assert 4 * cm <= bc.C[name] <= bc.round_up_1sig(4 * cm * 1.05), (name, cm, bc.round_up_1sig(4 * cm))
    # launch B: one lost or doubled update shows on at least half of the touched rows
    vis = {tab: bc.visibility(c, tab) for tab in ("UVB" if c.use_bias else "UV")}
    print("\n%s: %d triplets (%d skipped), %d clean (%.0f %%)%s, z 5..95 %% = %.2f..%.2f, %d ambiguous signs, max touches U %d V %d, "
          "float32 step error %.3g, c measured %.3g -> C = %.3g, single-update visibility %s" % (
              name, n_trip, c.skipped, n_clean, 100.0 * n_clean / n_trip,
              "" if n_hot_clean is None else ", %d with a hot positive" % n_hot_clean, z05, z95, ambiguous,
              c.touches["U"].max(), tv.max(), t32, cm, bc.round_up_1sig(4 * cm),
              ", ".join("%s %.2f" % kv for kv in vis.items())))
    if not c.only_b:  # (the wide-tile case alone may fall below: its comment says why)
        assert min(vis.values()) >= 0.5, vis
    if c.form == "owned":
        tu = c.touches["U"]
        assert tu[tu > 0].mean() < 4 and tv[tv > 0].mean() < 4, "few touches per row"
        assert c.shared.any() and not c.shared.all(), "exclusive users (plain stores) and shared ones (atomics) both occur"
        assert vis["U"] >= 0.5, vis


def test_t_clean_follows_its_rule(oracle):
    worst = max(_T32[name] if name in _T32 else _t32_measured(bc.case(name)) for name in bc.NAMES)
    print("\nfloat32 step vs float64 step over the clean rows of all cases: %.3g -> T_CLEAN = %.3g" % (worst, bc.round_up_1sig(4 * worst)))
    assert bc.T_CLEAN == bc.round_up_1sig(4 * worst)


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
    c = bc.case("fused_k7")  # k = 7: a lane group of 8 with one lane beyond k
    good = {lr: step.sequential(c.trip, c.tables, lr, bc.REG, True) for lr in (bc.LR_A, bc.LR_B)}
    return c, good


def test_the_unmutated_reference_passes_every_check(mutation_case):
    c, good = mutation_case
    bc.check_z(c, c.tables, int((c.x > 0).sum()), c.skipped)
    worst_a = bc.check_a(c, _as_device(good[bc.LR_A]))
    worst_b = bc.check_b(c, _as_device(good[bc.LR_B]))
    # the Jacobi sums (C) against the per-triplet deltas (numpy): two statements of the same update
    _, _, dU, dVi, dVj, dBi, dBj = step.deltas(c.trip, *c.tables, bc.LR_B, bc.REG, True)
    want_v, want_b = np.zeros(c.tables[1].shape), np.zeros(c.tables[2].shape)
    np.add.at(want_v, np.concatenate(c.trip[1:]), np.concatenate([dVi, dVj]))
    np.add.at(want_b, np.concatenate(c.trip[1:]), np.concatenate([dBi, dBj]))
    assert np.abs(want_v - c.jac["V"]["sum"]).max() <= 1e-15 and np.abs(want_b - c.jac["B"]["sum"]).max() <= 1e-15
    print("\nsequential float64 reference rounded to float32: A %s, B (error / tolerance) %s" % (worst_a, worst_b))


@pytest.mark.parametrize("mutant", MUTANTS)
def test_checks_reject_a_wrong_update(mutation_case, mutant):
    c, good = mutation_case
    out = {}
    for launch, lr in (("A", bc.LR_A), ("B", bc.LR_B)):
        if mutant in step.FAULTS:
            got = step.sequential(c.trip, c.tables, lr, bc.REG, True, fault=mutant)
        elif mutant == "row_written_to_the_wrong_item":
            got = tuple(t.copy() for t in good[lr])
            a, b = c.trip[1][np.flatnonzero(c.clean)[:2]]  # two touched item rows change places on the way back
            got[1][[a, b]] = got[1][[b, a]]
        else:
            tv = c.touches["V"]
            row = int(np.flatnonzero(tv == 3)[0])  # a row touched a few times, so not a clean one
            got = step.sequential(c.trip, c.tables, lr, bc.REG, True, **{"drop" if mutant == "one_update_lost" else "double": ("V", row)})
        check = bc.check_a if launch == "A" else bc.check_b
        out[launch] = _fails(check, c, _as_device(got))
    print("\n%s: rejected by %s" % (mutant, " and ".join(k for k, v in out.items() if v) or "NOTHING"))
    assert out["A"] or out["B"], mutant
    if mutant.startswith("one_update"):
        assert out["B"], "only launch B looks at rows touched more than once"
