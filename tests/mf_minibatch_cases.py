"""The minibatch MF step checks' cases, inputs and tolerance rule, in ONE place: tests/test_mf_minibatch_step_cpu.py holds the
rule's conditions on the two references alone, tests/test_mf_minibatch_step_gpu.py holds the device (`_lib.MfTrainer.
fit_minibatch`: csrc/mf_minibatch.inc) against the float64 reference.

References: oracle/mf_minibatch_oracle.fit, torch's own optimiser classes on the CPU, once over float32 tensors (what the
reference project computes) and once over float64 tensors with the device's float32-rounded scalars.

Tolerance of the device against the float64 run, per table (U, V, Bu, Bi):
    max(16 * d_ref, 4 units in the last float32 place of max|table|)
where d_ref = max|float32 run - float64 run| of that table of that case, computed when the test runs (cached per case).  It is
the rule of tests/ncf_cases.py for the same kind of comparison, not tuned on this kernel.  For every case and table that
tolerance must stay under 1 % of the table's movement max|float64 result - initial| (`check_condition`); a table that does not
move at all is compared bit for bit.  The call's summed squared error is held to max(16 * |float32 sum - float64 sum|,
1e-6 * float64 sum): the device sums in double and torch in float32, so on a short batch the first term can be almost 0.

Inputs come from numpy.random.RandomState: tables and biases float32 normal at scale 0.1, ratings 1..5, mu = 3.0.  In every
case but the conflict-free one user 0 appears in the first step only, the last item never appears, and item 1 fills a third of
every batch of five or more ratings.  A case is laid out position by position and then stored shuffled, so `order` is a
non-identity permutation of the rating arrays; "dup" cases repeat one rating index inside the second batch."""
import functools

import numpy as np

from oracle import mf_minibatch_oracle

OPTS = ("sgd", "adam", "rmsprop", "adagrad")
TABLES = ("U", "V", "Bu", "Bi")
MU = 3.0
ITEM = 1   # the item that fills a third of every batch
GRAD_STRIDE = 4096 * 16    # ratings per pass of mf_mb_grad_kernel's grid
APPLY_STRIDE = 8192 * 256  # table entries per pass of mf_mb_apply_kernel's grid
# one learning rate per optimiser; the batches of 70 000 ratings take a smaller one for SGD, whose step grows with the batch
LR = {"sgd": 0.01, "adam": 0.01, "rmsprop": 0.01, "adagrad": 0.05}
LR_BIG = dict(LR, sgd=2e-5)


def _c(nu, ni, k, n, bs, opt, reg, seed, lr=None, use_bias=True, dup=False, drop=None, distinct=False):
    return dict(nu=nu, ni=ni, k=k, n=n, bs=bs, opt=opt, lr=LR[opt] if lr is None else lr, reg=reg, seed=seed, use_bias=use_bias,
                dup=dup, drop=drop, distinct=distinct)


CASES = {}
for _q, _k in enumerate((1, 15, 16, 17, 32, 33, 100)):   # the gradient kernel's 16-lane stride over a row, ragged last batch of 33
    for _o, _opt in enumerate(OPTS):
        CASES["k%d/%s" % (_k, _opt)] = _c(37, 29, _k, 333, 50, _opt, 0.05 * ((_q + _o) % 2), 100 + 4 * _q + _o)
for _q, (_tag, _bs, _n) in enumerate((("b1", 1, 6), ("b15", 15, 52), ("b16", 16, 55), ("b17", 17, 58), ("dup", 17, 58))):
    for _o, _opt in enumerate(OPTS):
        CASES["%s/%s" % (_tag, _opt)] = _c(37, 29, 17, _n, _bs, _opt, 0.05 * ((_q + _o + 1) % 2), 140 + 4 * _q + _o, dup=_tag == "dup")
for _o, _opt in enumerate(OPTS):
    # mf_mb_grad_kernel's grid-stride loop: batches above 65 536 ratings (three of 70 000 and one of 1 000: four steps)
    CASES["gstride/%s" % _opt] = _c(300, 200, 3, 211000, 70000, _opt, 0.05 * (_o % 2), 170 + _o, lr=LR_BIG[_opt])
    # mf_mb_apply_kernel's: U alone is above 2 097 152 entries; its tail, V, Bu and Bi fall to the second pass
    CASES["astride/%s" % _opt] = _c(16500, 200, 128, 300, 64, _opt, 0.05 * ((_o + 1) % 2), 180 + _o)
    # segment ends inside a block and a wave (37 * 5 = 185) and on a block's end (32 * 8 = 256), with and without biases
    for _b in (True, False):
        _t = "" if _b else "/nobias"
        CASES["seg185/%s%s" % (_opt, _t)] = _c(37, 29, 5, 58, 17, _opt, 0.05 * (_o % 2), 190 + 2 * _o + _b, use_bias=_b)
        CASES["seg256/%s%s" % (_opt, _t)] = _c(32, 24, 8, 58, 17, _opt, 0.05 * ((_o + 1) % 2), 200 + 2 * _o + _b, use_bias=_b)
    # every gradient entry gets one atomic add: the users of a batch are distinct and so are its items
    CASES["distinct/%s" % _opt] = _c(37, 29, 17, 110, 29, _opt, 0.05 * (_o % 2), 210 + _o, distinct=True)
# dropout: masks per position of `order`, p = 0.3; ragged batches, a repeated index; one all-zero user mask and one all-zero
# item mask; the >65 536 positions for the masks' offsets; p = 1 as the model sends it (all-zero masks, keep_scale 0)
for _o, (_k, _opt) in enumerate(((1, "sgd"), (16, "adam"), (17, "rmsprop"), (33, "adagrad"))):
    CASES["drop/k%d/%s" % (_k, _opt)] = _c(37, 29, _k, 333, 50, _opt, 0.05 * (_o % 2), 220 + _o, dup=True, drop=0.3, use_bias=_o != 2)
for _o, _opt in enumerate(OPTS):
    CASES["drop/p1/%s" % _opt] = _c(37, 29, 17, 58, 17, _opt, 0.05, 230 + _o, dup=True, drop=1.0)
CASES["drop/gstride/adam"] = _c(300, 200, 3, 211000, 70000, "adam", 0.05, 240, drop=0.3)
CASES["drop/gstride/sgd"] = _c(300, 200, 3, 211000, 70000, "sgd", 0.0, 241, lr=LR_BIG["sgd"], drop=0.3)

STEP_CASES = sorted(n for n, c in CASES.items() if c["drop"] is None)
DROPOUT_CASES = sorted(n for n, c in CASES.items() if c["drop"] is not None)


def keeps_state(c):
    """the cases in which user 0's row goes on moving after its only gradient: Adam's first moment decays over the later
    steps whatever reg is; RMSprop's update is lr * g / (sqrt(square_avg) + eps), which without weight decay is 0 for a row
    whose gradient is 0, so its state shows only where reg > 0 (g = reg * w over the square_avg the first step left)"""
    return not c["distinct"] and c["drop"] is None and (c["opt"] == "adam" or (c["opt"] == "rmsprop" and c["reg"] > 0))


# ---- inputs ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(U, V, Bu, Bi, rid, cid, val, order, batches, keep, keep_u, keep_i, keep_scale), read-only"""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"])
    nu, ni, k, n, bs = c["nu"], c["ni"], c["k"], c["n"], c["bs"]
    d = {"U": rs.normal(0, .1, (nu, k)).astype(np.float32), "V": rs.normal(0, .1, (ni, k)).astype(np.float32),
         "Bu": rs.normal(0, .1, nu).astype(np.float32), "Bi": rs.normal(0, .1, ni).astype(np.float32)}
    users, items = np.empty(n, np.int64), np.empty(n, np.int64)
    for s, a in enumerate(range(0, n, bs)):   # position by position, batch by batch
        m = min(bs, n - a)
        if c["distinct"]:
            users[a:a + m], items[a:a + m] = rs.permutation(nu)[:m], rs.permutation(ni)[:m]
            continue
        users[a:a + m] = rs.randint(1, nu, m)
        if s == 0:
            users[a] = 0   # user 0: the first step only
        items[a:a + m] = rs.randint(0, ni - 1, m)   # the last item: never
        if m >= 5:
            items[a + rs.permutation(m)[:m // 3]] = ITEM
    vals = rs.randint(1, 6, n).astype(np.float32)
    order = rs.permutation(n).astype(np.int64)   # the rating of position b is stored at order[b]
    d["rid"], d["cid"], d["val"] = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.float32)
    d["rid"][order], d["cid"][order], d["val"][order] = users, items, vals
    if c["dup"]:
        order[bs + 2] = order[bs + 1]   # the same rating twice in the second batch (the rating stored at the old index rests)
    d["order"] = order
    d["batches"] = tuple(order[a:a + bs] for a in range(0, n, bs))
    d["keep"], d["keep_u"], d["keep_i"], d["keep_scale"] = None, None, None, 1.0
    if c["drop"] is not None:
        p = c["drop"]
        ku, ki = (rs.rand(n, k) >= p).astype(np.uint8), (rs.rand(n, k) >= p).astype(np.uint8)
        if p < 1.0:
            ku[bs + 3], ki[bs + 4] = 0, 0   # a position whose user row is dropped whole, one whose item row is
        d["keep_u"], d["keep_i"] = ku, ki
        d["keep_scale"] = float(np.float32(1.0) / np.float32(1.0 - p)) if p < 1.0 else 0.0
        d["keep"] = tuple((ku[a:a + bs], ki[a:a + bs]) for a in range(0, n, bs))
    for n, a in d.items():   # (the index arrays stay writable: torch wraps them without a copy and says so if they are not)
        if isinstance(a, np.ndarray) and n in TABLES + ("keep_u", "keep_i"):
            a.setflags(write=False)
    return d


def position_rows(name):
    """(users, items) of the positions of `order`"""
    d = inputs(name)
    return d["rid"][d["order"]], d["cid"][d["order"]]


# ---- references ------------------------------------------------------------------------------------------------------------
def oracle_fit(c, tables, d, batches, dtype, keep=None, opt=None, return_state=False):
    """mf_minibatch_oracle.fit over `batches` from `tables` with the case's arguments (mu is always passed: without biases the
    reference ignores it)"""
    return mf_minibatch_oracle.fit(*tables, MU, d["rid"], d["cid"], d["val"], batches, opt or c["opt"], c["lr"], c["reg"], c["use_bias"],
                                   keep=keep, keep_scale=d["keep_scale"], dtype=dtype, return_state=return_state)


def reference(name, dtype="float64", steps=None):
    """(U, V, Bu, Bi, summed loss) of the torch run over the first `steps` batches (None: all) in `dtype`; computed once,
    shared and read-only"""
    return _reference(name, dtype, steps)


@functools.lru_cache(maxsize=None)
def _reference(name, dtype, steps):
    c, d = CASES[name], inputs(name)
    keep = None if d["keep"] is None else d["keep"][:steps]
    out = oracle_fit(c, [d[t] for t in TABLES], d, d["batches"][:steps], np.dtype(dtype).type, keep)
    for a in out[:4]:
        a.setflags(write=False)
    return out[:4] + (float(np.sum(np.asarray(out[4], np.float64))),)


# ---- tolerances ------------------------------------------------------------------------------------------------------------
def ulp32(x):
    """(at 0: the smallest float32 step, 2^-149, written out: np.spacing there is a float32 denormal, which reads as 0 in a
    process where a library has switched denormals off)"""
    return max(float(np.spacing(np.float32(abs(x)))), 2.0 ** -149) if x else 2.0 ** -149


def tolerance(d_ref, top):
    """top: max|table|"""
    return max(16.0 * float(d_ref), 4.0 * ulp32(float(top)))


def table_tolerances(f32, f64):
    """per table of two runs of one problem: the rule's tolerance"""
    return [tolerance(np.abs(a.astype(np.float64) - b).max(), np.abs(b).max()) for a, b in zip(f32[:4], f64[:4])]


def loss_tolerance(sum32, sum64):
    return max(16.0 * abs(float(sum32) - float(sum64)), 1e-6 * float(sum64))


@functools.lru_cache(maxsize=None)
def tolerances(name):
    """(per-table tolerances, the loss's tolerance) of a case"""
    f32, f64 = reference(name, "float32"), reference(name, "float64")
    return tuple(table_tolerances(f32, f64)), loss_tolerance(f32[4], f64[4])


def movements(name):
    d, f64 = inputs(name), reference(name)
    return [float(np.abs(f64[q] - d[t].astype(np.float64)).max()) for q, t in enumerate(TABLES)]


def check_moves(tols, moves, f32, init, what):
    """the rule's condition on the references alone: every table's tolerance stays under 1 % of its movement; a table that
    does not move is one the float32 run leaves bit for bit too.  Returns the worst share."""
    worst = 0.0
    for q, t in enumerate(TABLES):
        if moves[q] == 0.0:
            assert np.array_equal(np.asarray(f32[q]).view(np.uint32), np.asarray(init[q], np.float32).view(np.uint32)), (what, t)
            continue
        worst = max(worst, tols[q] / moves[q])
        assert tols[q] <= 0.01 * moves[q], "%s %s: tolerance %.3g is not under 1 %% of the movement %.3g" % (what, t, tols[q], moves[q])
    return worst


def check_condition(name):
    d = inputs(name)
    return check_moves(tolerances(name)[0], movements(name), reference(name, "float32"), [d[t] for t in TABLES], name)


# ---- the model over the golden dataset's own batches -------------------------------------------------------------------------
MODEL_CASES = [(opt, use_bias, 0.0) for opt in OPTS for use_bias in (True, False)] + \
    [("sgd", True, 0.3), ("adam", True, 0.5), ("rmsprop", False, 0.2), ("adagrad", True, 0.1)]   # test_mf_minibatch.DROPOUT_CASES


@functools.lru_cache(maxsize=None)
def model_reference(opt, use_bias, p):
    """MF(backend="hip-minibatch")'s problem on the golden dataset as tests/test_mf_minibatch.py rebuilds it (the model's
    initial draw, the dataset's own shuffled batches, the reference's dropout draws), run by both torch modes: dict(fx, init,
    f32, f64, tols, moves)"""
    from conftest import load_golden
    from test_mf_minibatch import _setup

    fx = load_golden("mf_minibatch_dropout" if p else "mf_minibatch")
    ds, U, V, mu, rid, cid, val, batches = _setup(fx, use_bias)
    keep, scale = None, 1.0
    if p:
        keep, scale = mf_minibatch_oracle.dropout_masks(p, int(fx["seed"]), ds.num_users, ds.num_items, int(fx["k"]), use_bias,
                                                        [len(b) for b in batches])
    init = [U, V, np.zeros(ds.num_users, np.float32), np.zeros(ds.num_items, np.float32)]
    f32, f64 = (mf_minibatch_oracle.fit(*init, mu, rid, cid, val, batches, opt, float(fx["lr"]), float(fx["reg"]), use_bias, keep=keep,
                                        keep_scale=scale, dtype=dt) for dt in (np.float32, np.float64))
    moves = [float(np.abs(f64[q] - init[q].astype(np.float64)).max()) for q in range(4)]
    return dict(fx=fx, init=init, f32=f32, f64=f64, tols=table_tolerances(f32, f64), moves=moves)


def user0_movement(name):
    """how far user 0's row moves after the first step, its last gradient, in the float64 run"""
    return float(np.abs(reference(name)[0][0] - reference(name, "float64", 1)[0][0]).max())
