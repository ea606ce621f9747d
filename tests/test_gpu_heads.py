"""Every copy of the logistic head on the device, at saturated, tied and zero logits (tests/head_cases.py), against the
longdouble head of tests/head_ref.py.  The planted logits come back bit for bit; every probe's g is read from the fresh
Adam slots of its two bias entries and from its factor row; the loss sum, the sum of g and every inference are held to
the bounds of head_ref with ``step_ref.limit_from`` of the CPU stand-in's ratio as the limit.  The measured ratios are
printed as RATIO lines (run with -s), for DESIGN.md's table."""
import time

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import fm_cases
from tests import head_cases as C
from tests import step_ref as R
from tests.test_gpu_step_gradients import _plan_words

pytestmark = pytest.mark.gpu

SLOTS = (0, L.SLOT_M, L.SLOT_V)


def _finite(m, tids, adam):
    return all(bool(np.isfinite(m.get_table(tid | s)).all()) for tid in tids for s in (SLOTS if adam else (0,)))


def _g(m, tid, rows=None):
    a = m.get_table(tid | L.SLOT_M)
    return np.asarray(a if rows is None else a[rows], np.float64) / R.OMB1


def _report(tag, worst, t0):
    for what, v in sorted(worst.items()):
        print("RATIO %s %s: dev %.2f | c_ref %.2f" % (tag, what, v["dev"], v["c_ref"]))
    print("TIME %s %.1f s" % (tag, time.time() - t0))


def _hold(c, got, worst):
    rep = {}
    bad = C.check_training(c, got, rep)
    for what, v in rep.items():
        w = worst.setdefault(what, dict(dev=0.0, c_ref=0.0))
        w["dev"], w["c_ref"] = max(w["dev"], v["dev"]), max(w["c_ref"], v["c_ref"])
    assert not bad, "%s:\n  %s" % (c["id"], "\n  ".join(bad))


def _bias_and_rows(m, c, adam, tids):
    """the readings of a model with bu, bi, P and mu (SvdModel, SvdppModel)"""
    got = dict(finite=_finite(m, tids, adam))
    if adam:
        got.update(g_a=_g(m, L.BU, c["a_rows"]), g_b=_g(m, L.BI, c["b_rows"]), g_mu=float(_g(m, L.MU)),
                   g_rows=_g(m, L.P, c["a_rows"]) / c["qd"].astype(np.float64), v_a=m.get_table(L.BU | L.SLOT_V)[c["a_rows"]])
    return got


# ----------------------------------------------------------------------------- training heads
def _svd_step(cfg, c):
    _, _, U, I, D, B, opt, mode = cfg
    adam, t = opt == "adam", c["tables"]
    with T.SvdModel(U, I, D, loss="nll", item_abs=c["item_abs"], reg_bias=False, optimizer=opt, adam_mode=mode,
                    lr=C.ADAM_LR if adam else C.SGD_LR, reg=C.LAM) as m:
        m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
        logits, lossv, _ = m.train_step(c["u"], c["i"], c["z"])
        got = _bias_and_rows(m, c, adam, (L.MU, L.BU, L.BI, L.P, L.Q))
    got.update(logits=logits, loss=lossv)
    return got


def _svd_plan(cfg):
    name, path, U, I, D, B, opt, mode = cfg
    with T.SvdModel(U, I, D, loss="nll", optimizer=opt, adam_mode=mode) as m:
        plan = ";".join("%s=%s" % kv for kv in m.kernel_plan(B).items())
    for word in _plan_words(dict(path=path, D=D, opt=opt, mode=mode)):
        assert word in plan, "%s: %r not in the plan %r" % (name, word, plan)


@pytest.mark.parametrize("cfg", C.SVD_CONFIGS, ids=lambda c: c[0])
def test_svd_training_heads(cfg):
    """k_tile_step, k_front, k_forward TRAIN and k_seg_reduce's forward: sigmoidf_ - r and the cross-entropy line"""
    t0, worst = time.time(), {}
    _svd_plan(cfg)
    try:
        for c in C.svd_cases(cfg):
            _hold(c, _svd_step(cfg, c), worst)
    finally:
        _report(cfg[0], worst, t0)


def _fm_step(c, D, opt):
    adam, t = opt == "adam", c["tables"]
    with T.FmModel(c["F"], D, loss="nll", optimizer=opt, lr=C.ADAM_LR if adam else C.SGD_LR, reg=C.LAM) as m:
        m.set(t["mu"], t["W"], t["V"])
        pred, lossv = m.train_step(fm_cases.as_csr(c["csr"], c["F"]), c["z"])
        got = dict(logits=pred, loss=lossv, finite=_finite(m, (L.MU, L.BU, L.P), adam))
        if adam:
            got.update(g_a=_g(m, L.BU, c["a_rows"]), g_mu=float(_g(m, L.MU)), v_a=m.get_table(L.BU | L.SLOT_V)[c["a_rows"]])
    return got


@pytest.mark.parametrize("D", C.FM_DIMS)
def test_fm_training_heads(D):
    """csrc/fm_kernels.hip: a probe feature occurs in one row with W_f = 0, so m_W / (1 - b1) is that row's g"""
    t0, worst = time.time(), {}
    try:
        for c in C.fm_cases(D):
            _hold(c, _fm_step(c, D, "adam"), worst)
    finally:
        _report("fm-D%d" % D, worst, t0)


def _svdpp_step(c, D, opt):
    adam, t = opt == "adam", c["tables"]
    U, I = C.SVDPP_WORLD
    with T.SvdppModel(U, I, D, loss="nll", item_abs=c["item_abs"], reg_bias=False, optimizer=opt, adam_mode="lazy",
                      lr=C.ADAM_LR if adam else C.SGD_LR, reg=C.LAM) as m:
        m.set_tables(*(t[k] for k in ("mu", "bu", "bi", "P", "Q", "Y")))
        m.set_implicit(C.svdpp_implicit(U, I))
        logits, lossv, _ = m.train_step(c["u"], c["i"], c["z"])
        got = _bias_and_rows(m, c, adam, (L.MU, L.BU, L.BI, L.P, L.Q, L.Y))
    got.update(logits=logits, loss=lossv)
    return got


@pytest.mark.parametrize("D", C.SVDPP_DIMS)
def test_svdpp_training_heads(D):
    """csrc/svdpp.hip (expf): P = 0 and Y = 0 leave the effective user row zero"""
    t0, worst = time.time(), {}
    try:
        for c in C.svdpp_cases(D):
            _hold(c, _svdpp_step(c, D, "adam"), worst)
    finally:
        _report("svdpp-D%d" % D, worst, t0)


def _bpr_step(c, D, opt):
    adam, t = opt == "adam", c["tables"]
    U, I = C.BPR_WORLD
    pos = np.zeros(U, np.int32)
    pos[c["u"]] = c["i"]
    with T.SvdModel(U, I, D, item_abs=c["item_abs"], reg_bias=False, optimizer=opt, adam_mode="lazy",
                    lr=C.ADAM_LR if adam else C.SGD_LR, reg=C.LAM) as m:
        m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
        m.set_positives((np.arange(U + 1, dtype=np.int64), pos))
        neg, lossv, _, skipped = m.train_bpr_step(c["u"], c["i"], c["j"])
        assert np.array_equal(neg, c["j"]) and skipped == 0
        got = dict(logits=None, loss=lossv, finite=_finite(m, (L.MU, L.BU, L.BI, L.P, L.Q), adam))
        if adam:                                          # the positive's bi receives g, the negative's -g
            got.update(g_a=_g(m, L.BI, c["a_rows"]), g_b=-_g(m, L.BI, c["b_rows"]),
                       g_rows=_g(m, L.P, c["u"]) / c["qd"].astype(np.float64), v_a=m.get_table(L.BI | L.SLOT_V)[c["a_rows"]])
    return got


@pytest.mark.parametrize("D", C.BPR_DIMS)
def test_bpr_training_heads(D):
    """csrc/bpr.hip: -sigmoid(-x) and softplus(-x) on x = bi[i] - bi[j]"""
    t0, worst = time.time(), {}
    try:
        for c in C.bpr_cases(D):
            _hold(c, _bpr_step(c, D, "adam"), worst)
    finally:
        _report("bpr-D%d" % D, worst, t0)


@pytest.mark.parametrize("what", [c[0] for c in C.SVD_SGD_CONFIGS] + ["fm-sgd", "svdpp-sgd", "bpr-sgd"])
def test_sgd_steps_keep_the_logits_the_loss_and_finite_tables(what):
    """one SGD run per path, for the loss and finiteness only: a gradient read back as (w - w') / lr carries |w| / lr"""
    t0, worst = time.time(), {}
    try:
        if what == "fm-sgd":
            for c in C.fm_cases(16, ("mixed",)):
                _hold(c, _fm_step(c, 16, "sgd"), worst)
        elif what == "svdpp-sgd":
            for c in C.svdpp_cases(33, ("mixed",)):
                _hold(c, _svdpp_step(c, 33, "sgd"), worst)
        elif what == "bpr-sgd":
            for c in C.bpr_cases(33):
                _hold(c, _bpr_step(c, 33, "sgd"), worst)
        else:
            cfg = [c for c in C.SVD_SGD_CONFIGS if c[0] == what][0]
            _svd_plan(cfg)
            for c in C.svd_cases(cfg, ("mixed",)):
                _hold(c, _svd_step(cfg, c), worst)
    finally:
        _report(what, worst, t0)


# ----------------------------------------------------------------------------- eval heads
def _hold_eval(c, tag, **got):
    rep = {}
    bad = C.check_eval(c, report=rep, **got)
    for what, v in rep.items():
        print("RATIO %s %s %s: dev %.2f | c_ref %.2f" % (c["id"], tag, what, v["dev"], v["c_ref"]))
    assert not bad, "%s, %s:\n  %s" % (c["id"], tag, "\n  ".join(bad))


def test_svd_eval_heads():
    """binary_infer and sigmoid_xent in k_forward's evaluation mode and in k_forward_bf16: tfr_eval, tfr_eval_binary,
    tfr_eval_binary_resident, tfr_eval_resident, tfr_bf16_eval.  30001 entries are more than one grid: the grid-stride
    loop runs.  No flip allowance: the tie probes are in the set with both labels."""
    c = C.eval_case("svd", 30001)
    t, n = c["tables"], c["x"].size
    u, i, z = c["u"], c["i"], c["z"]
    with T.SvdModel(c["U"], c["I"], c["D"], loss="nll") as m:
        m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
        assert R.same_bits(m.forward(u, i), c["x"])
        sse, neq = m.eval(u, i, z)
        _hold_eval(c, "eval", n_equal=neq, sse=sse)
        e = m.eval_binary(u, i, z)
        assert e["n"] == n
        _hold_eval(c, "eval_binary", n_equal=int(round(e["acc"] * n)), nll_sum=e["mean_nll"] * n)
        m.upload_eval_triples(u, i, z)
        e = m.eval_binary_resident()
        assert e["n"] == n
        _hold_eval(c, "eval_binary_resident", n_equal=int(round(e["acc"] * n)), nll_sum=e["mean_nll"] * n)
        sse, neq, cnt = m.eval_resident()
        assert cnt == n
        _hold_eval(c, "eval_resident", n_equal=neq, sse=sse)
        m.snapshot_bf16()                                 # every planted value survives the round trip to bf16
        assert R.same_bits(m.forward_bf16(u, i), c["x"])
        sse, neq, nll = m.eval_bf16(u, i, z)
        _hold_eval(c, "eval_bf16", n_equal=neq, sse=sse, nll_sum=nll)


def test_svdpp_eval_heads():
    c = C.eval_case("svdpp", 30001)
    t = c["tables"]
    with T.SvdppModel(c["U"], c["I"], c["D"], loss="nll") as m:
        m.set_tables(*(t[k] for k in ("mu", "bu", "bi", "P", "Q", "Y")))
        m.set_implicit(C.svdpp_implicit(c["U"], c["I"]))
        assert R.same_bits(m.forward(c["u"], c["i"]), c["x"])
        sse, neq = m.eval(c["u"], c["i"], c["z"])
        _hold_eval(c, "svdpp_eval", n_equal=neq, sse=sse)


def test_fm_eval_heads():
    """csrc/fm_fit.hip: the resident store's predictions and its metrics"""
    c = C.eval_case("fm", 5000)
    t, n = c["tables"], c["x"].size
    with T.FmModel(c["F"], c["D"], loss="nll") as m:
        m.set(t["mu"], t["W"], t["V"])
        m.upload_rows(fm_cases.as_csr(c["csr"], c["F"]), c["z"], "eval")
        assert R.same_bits(m.predict_resident("eval"), c["x"])
        e = m.eval_binary_resident()
        assert e["n"] == n
        _hold_eval(c, "fm_eval_binary_resident", n_equal=int(round(e["acc"] * n)), nll_sum=e["mean_nll"] * n)
