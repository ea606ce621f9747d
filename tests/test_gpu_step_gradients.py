"""Every SVD step path, per row: the gradient sum the device used, its Adam moments and its apply, each held to its own
tight statement (tests/step_ref.py) instead of "the table is near the oracle's".  Two successive steps on a fresh model;
P, Q, bu, bi, mu and their m and v are read before, between and after.  The cases (tests/step_cases.py) name the step path
they were written for, and ``kernel_plan`` is held against it."""
import ctypes
import time

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from oracle import svd_oracle as so
from tests import step_cases as S
from tests import step_ref as R
from tests.util import RTOL, assert_close

pytestmark = pytest.mark.gpu


def _snapshot(m, adam):
    out = {}
    for name in R.NAMES:
        tid = R.TID[name]
        d = dict(w=m.get_table(tid))
        if adam:
            d["m"], d["v"] = m.get_table(tid | L.SLOT_M), m.get_table(tid | L.SLOT_V)
        out[name] = d
    return out


def _plan_words(case):
    """what kernel_plan must say for the path a case names (csrc/api.hip tfr_kernel_plan)"""
    path, D = case["path"], case["D"]
    vec = 4 if D % 4 == 0 else 1
    lanes, g = -(-D // vec), 4
    while g < lanes:
        g *= 2
    if path.startswith("tiles"):
        return ["reduce_item=k_tile_step<%d, %d, " % (g, vec), "apply=k_dense_tiles<%d, %d, false, %s>" % (g, vec, path[5:])]
    if path == "csort":
        return ["forward=k_front<%d, %d>" % (g, vec), "sort=k_csort_scan/scatter",
                "apply=k_adam_dense" if case["mode"] == "tf1" and case["opt"] == "adam" else "apply=k_apply_rows"]
    if path.startswith("tf1"):
        return ["forward=k_forward<", "sort=k_rsort_rank/scan/scatter", "apply=k_adam_dense<%d, %d>" % (g, vec), "finalize=k_finalize"]
    fast = "true" if D == g * vec else "false"            # the three-round load form takes full-width rows only
    rm = 1 if case["opt"] == "adam" else 2                # RMODE_ADAM / RMODE_SGD (csrc/svd_kernels.h)
    return ["sort=k_rsort", "reduce_item=k_seg_reduce<%d, %d, %d, true, true, %s>" % (g, vec, rm, fast),
            "reduce_user=k_seg_reduce<%d, %d, %d, false, true, %s>" % (g, vec, rm, fast), "apply=k_apply_rows<%d, %d, " % (g, vec)]


def _check_two_steps(case, report=None):
    U, I, D, B = case["U"], case["I"], case["D"], case["B"]
    adam = case["opt"] == "adam"
    flags = dict(loss=case["loss"], item_abs=case["item_abs"], reg_bias=case["reg_bias"])
    lr, reg = S.hyper_of(case, 0)
    t = S.tables_of(case)
    with T.SvdModel(U, I, D, optimizer=case["opt"], adam_mode=case["mode"], lr=lr, reg=reg, **flags) as m:
        m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
        if case["frozen"]:
            m.set_frozen(case["frozen"])
        plan = ";".join("%s=%s" % kv for kv in m.kernel_plan(B).items())      # phase=kernel, as tfr_kernel_plan writes it
        for word in _plan_words(case):                                 # 1. the path the case was written for
            assert word in plan, "%s: %r not in the plan %r" % (case["id"], word, plan)
        assert m.get_step()[0] == 0
        before = _snapshot(m, adam)
        for s in range(2):
            if s == 1 and case["hyper2"]:
                m.set_hyper(*case["hyper2"])
            lr, reg = S.hyper_of(case, s)
            u, i, r = S.batch_of(case, s)
            _, b1p, b2p = m.get_step()
            logits, lossv, regv = m.train_step(u, i, r)
            after = _snapshot(m, adam)
            assert m.get_step()[0] == s + 1
            rep = {} if report is not None else None
            bad = R.check_step(before, after, u, i, r, opt=case["opt"], mode=case["mode"], lam=reg, lr=lr, powers=(b1p, b2p),
                               fresh=s == 0, frozen=case["frozen"], sample=case["sample"], report=rep, **flags)   # 2. - 6.
            if report is not None:
                report["step%d" % s] = rep
            assert not bad, "%s, step %d:\n  %s" % (case["id"], s, "\n  ".join(bad))
            # 7. logits, loss and regulariser against float64 on the tables the device started the step from
            w = R.f64_tables({k: before[k]["w"] for k in R.NAMES})
            x = so.forward(w["P"], w["Q"], w["bu"], w["bi"], w["mu"], u.astype(np.int64), i.astype(np.int64), case["item_abs"])
            tol = 2 * RTOL * (s + 1)
            assert_close(logits, x, rtol=tol, what="step %d logits" % s)
            assert_close(lossv, so.data_loss(x, r.astype(np.float64), case["loss"]), rtol=tol, what="step %d loss" % s)
            assert_close(regv, so.regularizer(w["P"], w["Q"], w["bu"], w["bi"], u, i, case["reg_bias"]), rtol=tol, what="step %d reg" % s)
            before = after


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c["id"])
def test_two_steps_per_row(case):
    t0 = time.time()
    report = {}
    try:
        _check_two_steps(case, report)
    finally:
        # the measured ratios (device and float32 oracle, per table and run-length class), for DESIGN.md's table
        for step, rep in sorted(report.items()):
            for name, v in rep.items():
                print("RATIO %s %s %s dev short %.2f long %.2f | c_ref short %.2f long %.2f" % (
                    case["id"], step, name, v["dev"]["short"], v["dev"]["long"], v["c_ref"]["short"], v["c_ref"]["long"]))
        print("TIME %s %.1f s" % (case["id"], time.time() - t0))


# tfr_kernel_plan's whole string on the four branches it has (csrc/api.hip), as it stood before the launchers took their
# instantiations from csrc/dispatch.h: bench.py looks the kernels of a step up by these strings, byte for byte.
PLAN_STRINGS = [
    (dict(U=500, I=500, D=16, adam_mode="tf1"), 3000,
     "reduce_item=k_tile_step<4, 4, 1>;apply=k_dense_tiles<4, 4, false, 4>"),
    (dict(U=500, I=500, D=16, adam_mode="tf1"), 20000,                         # beyond 16 tiles
     "forward=k_front<4, 4>;sort=k_csort_scan/scatter;reduce_item=k_seg_reduce<4, 4, 0, false, true, false>;apply=k_adam_dense"),
    (dict(U=40000, I=3000, D=64, adam_mode="lazy"), 4096,                      # one side above CSORT_MAX_BINS rows
     "sort=k_rsort_rank/scan/scatter x2 passes (the first gathers the batch);reduce_item=k_seg_reduce<16, 4, 1, true, true, true>;"
     "reduce_user=k_seg_reduce<16, 4, 1, false, true, true>;apply=k_apply_rows<16, 4, 0>"),
    (dict(U=40000, I=3000, D=25, optimizer="sgd"), 4096,
     "sort=k_rsort_rank/scan/scatter x2 passes (the first gathers the batch);reduce_item=k_seg_reduce<32, 1, 2, true, true, false>;"
     "reduce_user=k_seg_reduce<32, 1, 2, false, true, false>;apply=k_apply_rows<32, 1, 1>"),
]


@pytest.mark.parametrize("model,B,want", PLAN_STRINGS, ids=["tiles", "csort", "fused-lazy-adam", "fused-sgd"])
def test_kernel_plan_strings_are_pinned(model, B, want):
    kw = {k: v for k, v in model.items() if k not in ("U", "I", "D")}
    buf = ctypes.create_string_buffer(1024)                # the raw string: SvdModel.kernel_plan hands back a dict of it
    with T.SvdModel(model["U"], model["I"], model["D"], **kw) as m:
        L.check(m._lib.tfr_kernel_plan(m._h, B, buf, 1024))
    assert buf.value.decode() == want
