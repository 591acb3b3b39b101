"""`MF(backend="hip-minibatch")`'s optimiser steps on the device (csrc/mf_minibatch.inc through `_lib.MfTrainer`) against torch's
own optimisers run in float64 (oracle/mf_minibatch_oracle.fit, dtype=np.float64), over the cases of tests/mf_minibatch_cases.py.

Every table (U, V, Bu, Bi) is held to
    max(16 * d_ref, 4 units in the last float32 place of max|table|),
d_ref = max|float32 torch - float64 torch| of that table of that case, computed when the test runs; that tolerance stays under
1 % of the table's movement (tests/test_mf_minibatch_step_cpu.py); a table that does not move is compared bit for bit.  A call's
summed squared error is held to max(16 * |float32 sum - float64 sum|, 1e-6 * float64 sum).  Every check prints the measured
difference next to its tolerance.

What these tests found: the host rounded Adam's 1 - beta2 and RMSprop's 1 - alpha in float32 arithmetic (1.f - 0.999f), 1.3e-5
below the (float)(1.0 - 0.999) that torch hands its tensor operations.  Every early Adam step was 6.4e-6 off in size: 2e-7 to
1e-6 after four to seven steps, up to 3.6 tolerances (b1/adam Bu), 35 tests of this file failing; RMSprop reached 1.26 tolerances
(k100/rmsprop V).  csrc/mf_minibatch.inc now rounds as torch does; the figures below are from after that.

Measured on an MI355X, over the 76 step cases and the 10 dropout cases: the device's worst difference as a share of its
tolerance U 0.30, V 0.47, Bu 0.16, Bi 0.37 (model level, 12 runs: 0.18); the worst loss 0.053 of its tolerance, 5.2e-08
relative.  User 0's row moved 3 800 to 85 000 tolerances after its last gradient (27 Adam and weight-decayed RMSprop cases) and
ended within 0.063 of a tolerance of the reference; the last item's row moved 650 to 470 000 tolerances by weight decay alone.
The worst tolerance / movement over all cases and tables is 1.7e-03 (astride/adagrad U).  Two runs of the conflict-free epoch
gave the same bits in all four tables under each of the four optimisers.  (d_ref comes from float32 torch on the machine that
runs the test and differs between machines by up to 3.4 times on the 2 112 000-entry table; the shares move with it.)
"""
import functools

import numpy as np
import pytest

import mf_minibatch_cases as mc
from cornac_amd import MF, _lib

pytestmark = pytest.mark.gpu
T = mc.TABLES


class trainer:
    """a device handle over a case's ratings, loaded with `tables` (None: the case's own), closed when the block ends"""

    def __init__(self, name, tables=None, val=None):
        c, d = mc.CASES[name], mc.inputs(name)
        self.tr = _lib.MfTrainer(d["rid"], d["cid"], d["val"] if val is None else val, c["nu"], c["ni"], c["k"])
        self.tr.set_factors(*(tables or [d[t] for t in T]))

    def __enter__(self):
        return self.tr

    def __exit__(self, *exc):
        self.tr.close()


def step(tr, name, order=None, opt=None, lo=0, hi=None, **over):
    """fit_minibatch over positions [lo, hi) of the case's order (or over `order`) with the case's arguments; the call's loss"""
    c, d = mc.CASES[name], mc.inputs(name)
    opt = opt or c["opt"]
    kw = dict(batch_size=c["bs"], lr=c["lr"] if opt == c["opt"] else mc.LR.get(opt, c["lr"]), reg=c["reg"], mu=mc.MU, use_bias=c["use_bias"])
    kw.update(over)
    keep = {}
    if d["keep_u"] is not None and order is None:
        keep = dict(keep_u=d["keep_u"][lo:hi], keep_i=d["keep_i"][lo:hi], keep_scale=d["keep_scale"])
    order = d["order"][lo:hi] if order is None else order
    return tr.fit_minibatch(order, kw["batch_size"], opt, kw["lr"], kw["reg"], kw["mu"], kw["use_bias"], **keep)


def run(name, val=None):
    with trainer(name, val=val) as tr:
        sse = step(tr, name)
        return tr.get_factors() + (sse,)


@functools.lru_cache(maxsize=None)
def device_run(name):
    """(U, V, Bu, Bi, summed loss) of one call over the whole case; computed once, shared and read-only"""
    out = run(name)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(what, got, want, tols, rows=None):
    """the device's tables against the float64 run's under the rule (rows: of that row only); the shares of the tolerance"""
    shares = []
    for q, t in enumerate(T):
        a, b = (got[q], want[q]) if rows is None or rows[q] is None else (got[q][rows[q]], want[q][rows[q]])
        assert got[q].dtype == np.float32 and np.isfinite(got[q]).all(), (what, t)
        d = float(np.abs(a.astype(np.float64) - b).max())
        shares.append(d / tols[q])
        print("SHARE %s %s: %.3g (tolerance %.3g) = %.3g" % (what, t, d, tols[q], d / tols[q]))
        assert d <= tols[q], (what, t, d, tols[q])
    return shares


def compare_case(name, got, what=""):
    """a whole case: the four tables, the tables that do not move bit for bit, and the loss"""
    d, want = mc.inputs(name), mc.reference(name)
    tols, ltol = mc.tolerances(name)
    compare(name + what, got, want, tols)
    for q, move in enumerate(mc.movements(name)):
        if move == 0.0:
            assert np.array_equal(bits(got[q]), bits(d[T[q]])), (name, T[q])
    dl = abs(got[4] - want[4])
    print("LOSS %s%s: %.6g against %.6g: off by %.3g (tolerance %.3g) = %.3g" % (name, what, got[4], want[4], dl, ltol, dl / ltol))
    assert np.isfinite(got[4]) and dl <= ltol, (name, got[4], want[4], ltol)


# ---- steps against the float64 reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.STEP_CASES)
def test_steps_against_the_float64_reference(name):
    c, d = mc.CASES[name], mc.inputs(name)
    got = device_run(name)
    compare_case(name, got)
    if not c["use_bias"]:   # called with mu = 3.0: mu, Bu and Bi stay out of it
        assert np.array_equal(bits(got[2]), bits(d["Bu"])) and np.array_equal(bits(got[3]), bits(d["Bi"]))


# ---- state seen through its effects ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, c in mc.CASES.items() if mc.keeps_state(c)))
def test_user0_row_moves_by_its_state_alone_and_stays_with_the_reference(name):
    tol, move = mc.tolerances(name)[0][0], mc.user0_movement(name)
    got, want = device_run(name)[0][0], mc.reference(name)[0][0]
    d = float(np.abs(got.astype(np.float64) - want).max())
    print("USER0 %s: moved %.3g after its last gradient = %.0f tolerances; device off by %.3g (tolerance %.3g)" % (name, move, move / tol, d, tol))
    assert move > 100 * tol and d <= tol


@pytest.mark.parametrize("name", ["k16/rmsprop", "k32/rmsprop", "b17/rmsprop"])
def test_rmsprop_without_weight_decay_leaves_user0_where_step_1_put_it(name):
    """(lr * 0 / (sqrt(square_avg) + eps): a row without a gradient rests, whatever its state holds)"""
    c = mc.CASES[name]
    assert c["reg"] == 0 and c["opt"] == "rmsprop"
    with trainer(name) as tr:
        step(tr, name, hi=c["bs"])
        first = tr.get_factors()[0][0].copy()
        step(tr, name, lo=c["bs"])
        last = tr.get_factors()[0][0]
    assert np.array_equal(bits(first), bits(last)) and not np.array_equal(bits(first), bits(mc.inputs(name)["U"][0]))


@pytest.mark.parametrize("name", [n for n in mc.STEP_CASES if not mc.CASES[n]["distinct"]])
def test_the_last_item_has_no_gradient(name):
    """reg = 0: its row and its bias keep their bits under every optimiser (Adam: 0 / (0 + eps)); reg > 0: the update is
    dense, the row moves by weight decay and stays within tolerance"""
    c, d = mc.CASES[name], mc.inputs(name)
    got, want, tols = device_run(name), mc.reference(name), mc.tolerances(name)[0]
    if c["reg"] == 0:
        assert np.array_equal(bits(got[1][-1]), bits(d["V"][-1])) and bits(got[3][-1:]) == bits(d["Bi"][-1:])
        return
    moved = float(np.abs(want[1][-1] - d["V"][-1].astype(np.float64)).max())
    print("LAST ITEM %s: the reference's row moves %.3g = %.0f tolerances" % (name, moved, moved / tols[1]))
    assert moved > tols[1] and not np.array_equal(bits(got[1][-1]), bits(d["V"][-1]))
    compare(name + " last item", got, want, tols, rows=(None, -1, None, -1))
    if c["use_bias"]:
        assert bits(got[3][-1:]) != bits(d["Bi"][-1:])


# ---- calls compose -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", mc.OPTS)
def test_two_calls_are_one_run(opt):
    """fit(A) then fit(B) = the reference over A + B: the state and Adam's step counter persist"""
    name = "k17/" + opt
    c = mc.CASES[name]
    with trainer(name) as tr:
        sse = step(tr, name, hi=2 * c["bs"]) + step(tr, name, lo=2 * c["bs"])
        compare_case(name, tr.get_factors() + (sse,), " in two calls")


@functools.lru_cache(maxsize=None)
def restarted(name, opt2, dtype):
    """the torch run over the case's first two batches, then a new optimiser `opt2` over the rest from those tables"""
    c, d = mc.CASES[name], mc.inputs(name)
    a = mc.oracle_fit(c, [d[t] for t in T], d, d["batches"][:2], np.dtype(dtype).type)
    return mc.oracle_fit(dict(c, lr=mc.LR[opt2]), list(a[:4]), d, d["batches"][2:], np.dtype(dtype).type, opt=opt2)


@pytest.mark.parametrize("opt,opt2", [("adam", "adam"), ("adam", "rmsprop"), ("rmsprop", "adagrad"), ("adagrad", "adam"), ("sgd", "adam"),
                                      ("rmsprop", "sgd")])
def test_reset_optimizer_starts_a_new_optimiser(opt, opt2):
    name = "k17/" + opt
    c, d = mc.CASES[name], mc.inputs(name)
    f32, f64 = restarted(name, opt2, "float32"), restarted(name, opt2, "float64")
    tols = mc.table_tolerances(f32, f64)
    moves = [float(np.abs(f64[q] - d[t].astype(np.float64)).max()) for q, t in enumerate(T)]
    mc.check_moves(tols, moves, f32, [d[t] for t in T], (name, opt2))
    with trainer(name) as tr:
        step(tr, name, hi=2 * c["bs"])
        tr.reset_optimizer()
        step(tr, name, opt=opt2, lo=2 * c["bs"])
        compare("%s then reset then %s" % (name, opt2), tr.get_factors(), f64, tols)


def test_an_empty_order_is_no_step():
    name = "k17/adam"
    c, d = mc.CASES[name], mc.inputs(name)
    empty = np.zeros(0, np.int64)
    with trainer(name) as tr:   # returns 0.0, moves nothing, pins no optimiser, advances no step
        assert step(tr, name, order=empty, opt="sgd") == 0.0
        assert all(np.array_equal(bits(a), bits(d[t])) for a, t in zip(tr.get_factors(), T))
        sse = step(tr, name, hi=2 * c["bs"])
        before = tr.get_factors()
        assert step(tr, name, order=empty) == 0.0
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(tr.get_factors(), before))
        sse += step(tr, name, lo=2 * c["bs"])
        compare_case(name, tr.get_factors() + (sse,), " around empty calls")


# ---- reproducibility where the code promises it ----------------------------------------------------------------------------
@pytest.mark.parametrize("opt", mc.OPTS)
def test_a_conflict_free_epoch_gives_the_same_bits_twice(opt):
    """users all distinct and items all distinct in every batch: one atomic add per gradient entry, no order to differ in"""
    name = "distinct/" + opt
    first, again = device_run(name), run(name)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first[:4], again[:4])) and first[4] == again[4]
    print("SAME BITS %s: two runs of the conflict-free epoch gave the same bits in all four tables" % name)


# ---- dropout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.DROPOUT_CASES)
def test_dropout_against_the_float64_reference_with_the_same_masks(name):
    """the masks belong to the positions of `order` (a permutation with a repeated index), not to the ratings"""
    compare_case(name, device_run(name))


@pytest.mark.parametrize("opt", mc.OPTS)
def test_dropout_of_everything_trains_the_biases_only(opt):
    """p = 1 as the model sends it (all-zero masks, keep_scale 0): the factor tables move by weight decay alone, so other
    ratings give them the same bits, while the biases follow the ratings"""
    name = "drop/p1/" + opt
    d, tols = mc.inputs(name), mc.tolerances(name)[0]
    got, other = device_run(name), run(name, val=(6.0 - d["val"]).astype(np.float32))
    assert np.array_equal(bits(got[0]), bits(other[0])) and np.array_equal(bits(got[1]), bits(other[1]))
    assert not np.array_equal(bits(got[0]), bits(d["U"])) and not np.array_equal(bits(got[1]), bits(d["V"]))
    for q in (2, 3):
        apart = float(np.abs(got[q].astype(np.float64) - other[q]).max())
        print("P1 %s %s: the two ratings' biases end %.3g apart = %.0f tolerances" % (name, T[q], apart, apart / tols[q]))
        assert apart > 100 * tols[q]


# ---- rejected calls change nothing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k17/adam", "k17/sgd", "drop/k17/rmsprop"])
def test_rejected_calls_change_nothing(name):
    c, d = mc.CASES[name], mc.inputs(name)
    n, bs, half = c["n"], c["bs"], 2 * c["bs"]
    other = mc.OPTS[(mc.OPTS.index(c["opt"]) + 1) % 4]
    bad_lo, bad_hi = d["order"][:bs].copy(), d["order"][:bs].copy()
    bad_lo[bs // 2], bad_hi[bs // 2] = -1, n
    masks = dict(keep_u=np.ones((bs, c["k"]), np.uint8), keep_i=np.ones((bs, c["k"]), np.uint8))
    with trainer(name) as tr:
        sse = step(tr, name, hi=half)
        before = tr.get_factors()
        tr.OPTIMIZERS = dict(tr.OPTIMIZERS, above=4, below=-1)
        rejected = [
            (_lib.HipError, r"order\[%d\] out of range" % (bs // 2), lambda: step(tr, name, order=bad_lo)),
            (_lib.HipError, r"order\[%d\] out of range" % (bs // 2), lambda: step(tr, name, order=bad_hi)),
            (_lib.HipError, r"order\[%d\] out of range" % (bs // 2),
             lambda: tr.fit_minibatch(bad_hi, bs, c["opt"], c["lr"], c["reg"], mc.MU, c["use_bias"], **masks)),
            (_lib.HipError, "batch_size must be positive", lambda: step(tr, name, hi=bs, batch_size=0)),
            (_lib.HipError, "unknown optimizer 4", lambda: step(tr, name, hi=bs, opt="above")),
            (_lib.HipError, "unknown optimizer -1", lambda: step(tr, name, hi=bs, opt="below")),
            (_lib.HipError, "optimizer changed mid-training; call cornac_hip_mf_reset_optimizer first", lambda: step(tr, name, hi=bs, opt=other)),
            (ValueError, "keep masks must be", lambda: tr.fit_minibatch(d["order"][:bs], bs, c["opt"], c["lr"], c["reg"], mc.MU, c["use_bias"],
                                                                         keep_u=masks["keep_u"][:-1], keep_i=masks["keep_i"][:-1])),
            (ValueError, "keep masks must be", lambda: tr.fit_minibatch(d["order"][:bs], bs, c["opt"], c["lr"], c["reg"], mc.MU, c["use_bias"],
                                                                         keep_u=masks["keep_u"], keep_i=masks["keep_i"][:, :-1])),
        ]
        for err, words, call in rejected:
            with pytest.raises(err, match=words):
                call()
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(tr.get_factors(), before)), words
        sse += step(tr, name, lo=half)   # no half-taken step remains: the rest of the case still ends at the reference
        compare_case(name, tr.get_factors() + (sse,), " after rejected calls")


# ---- model level -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,use_bias,p", mc.MODEL_CASES)
def test_model_against_the_float64_reference_over_the_golden_batches(opt, use_bias, p):
    """the runs that tests/test_mf_minibatch.py holds to 1e-4 / 2e-5 of the goldens, held by the rule to torch in float64 over
    the same batches and the same dropout draws (the tolerances are listed in tests/test_mf_minibatch_step_cpu.py)"""
    from conftest import golden_dataset

    ref = mc.model_reference(opt, use_bias, p)
    fx = ref["fx"]
    m = MF(k=int(fx["k"]), backend="hip-minibatch", optimizer=opt, max_iter=int(fx["epochs"]), batch_size=int(fx["batch_size"]),
           learning_rate=float(fx["lr"]), lambda_reg=float(fx["reg"]), use_bias=use_bias, dropout=p, seed=int(fx["seed"])).fit(golden_dataset(fx))
    got = [np.asarray(a) for a in (m.u_factors, m.i_factors, m.u_biases, m.i_biases)]
    compare("model %s bias %s p %s" % (opt, use_bias, p), got, ref["f64"], ref["tols"])
    if not use_bias:
        assert not got[2].any() and not got[3].any()
