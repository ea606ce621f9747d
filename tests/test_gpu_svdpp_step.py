"""The SVD++ training step, per row: the gradient sum the device used for P, Q, bu, bi, mu and Y, its Adam moments and its
apply, each held to its own statement (tests/svdpp_step_ref.py), the step's logits per entry, its data loss and its
regulariser.  Two successive steps on a fresh model; every table and its m and v are read before, between and after.  The
cases are tests/svdpp_cases.py: every piece, window and run edge of csrc/svdpp.hip, every frozen bit, sign(0)."""
import time

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import step_ref as R
from tests import svdpp_cases as C
from tests import svdpp_step_ref as S
from tests import widths as W

pytestmark = pytest.mark.gpu

assert {c["D"] for c in C.CASES if c["kind"] == "edges"} >= set(W.SVDPP)


def _snapshot(m, adam):
    out = {}
    for name in S.NAMES:
        tid = S.TID[name]
        d = dict(w=m.get_table(tid))
        if adam:
            d["m"], d["v"] = m.get_table(tid | L.SLOT_M), m.get_table(tid | L.SLOT_V)
        out[name] = d
    return out


def _model(case):
    lr, lam = C.hyper_of(case, 0)
    t = C.tables_of(case)
    m = T.SvdppModel(C.U, C.I, case["D"], loss=case["loss"], item_abs=case["item_abs"], reg_bias=case["reg_bias"],
                     optimizer=case["opt"], adam_mode="lazy", lr=lr, reg=lam)
    m.set_tables(*(t[k] for k in ("mu", "bu", "bi", "P", "Q", "Y")))
    m.set_implicit(C.implicit())
    if case["frozen"]:
        m.set_frozen(case["frozen"])
    return m


def _check_two_steps(case, report):
    adam = case["opt"] == "adam"
    N = C.implicit()
    with _model(case) as m:
        assert m.get_step()[0] == 0
        before = _snapshot(m, adam)
        for s in range(2):
            if s == 1 and case["hyper2"]:
                m.set_hyper(*case["hyper2"])
            lr, lam = C.hyper_of(case, s)
            u, i, r = C.batch_of(case, s)
            _, b1p, b2p = m.get_step()
            logits, lossv, regv = m.train_step(u, i, r)
            after = _snapshot(m, adam)
            assert m.get_step()[0] == s + 1
            rep = report.setdefault("step%d" % s, {})
            t0 = time.time()
            bad = S.check_svdpp_step(before, after, N, u, i, r, opt=case["opt"], loss=case["loss"], item_abs=case["item_abs"],
                                     reg_bias=case["reg_bias"], lam=lam, lr=lr, powers=(b1p, b2p), fresh=s == 0,
                                     frozen=case["frozen"], logits=logits, lossv=lossv, regv=regv, report=rep)
            print("TIME %s step%d NumPy reference and checks %.1f s" % (case["id"], s, time.time() - t0))
            assert not bad, "%s, step %d:\n  %s" % (case["id"], s, "\n  ".join(bad))
            before = after


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_two_svdpp_steps_per_row(case):
    t0 = time.time()
    report = {}
    try:
        _check_two_steps(case, report)
    finally:
        # the measured ratios (device and float32 restatement, per table and run-length class), for DESIGN.md's table
        for step, rep in sorted(report.items()):
            for name, v in rep.items():
                print("RATIO %s %s %s dev short %.2f long %.2f | c_ref short %.2f long %.2f" % (
                    case["id"], step, name, v["dev"]["short"], v["dev"]["long"], v["c_ref"]["short"], v["c_ref"]["long"]))
        print("TIME %s %.1f s" % (case["id"], time.time() - t0))


@pytest.mark.parametrize("case", [c for c in C.CASES if c["tail"] == 65 or c["kind"] == "edges" and c["D"] == 33],
                         ids=lambda c: c["id"])
def test_train_step_dev_equals_train_step_bit_for_bit(case):
    """tfr_svdpp_train_step_dev on device columns, the first step without a logits buffer and the second with one: every
    table and slot, and the logits, equal those of tfr_svdpp_train_step on the same host columns"""
    torch = pytest.importorskip("torch")
    adam = case["opt"] == "adam"
    snaps, logits = {}, {}
    for how in ("host", "dev"):
        with _model(case) as m:
            for s in range(2):
                u, i, r = C.batch_of(case, s)
                if how == "host":
                    logits[how] = m.train_step(u, i, r)[0]
                    continue
                d = [torch.from_numpy(a).cuda() for a in (u, i, r)]
                out = m.train_step_dev(*d, want_logits=s == 1)
                m.sync()
                torch.cuda.synchronize()
                logits[how] = out.cpu().numpy() if s == 1 else None
            assert m.get_step()[0] == 2
            snaps[how] = _snapshot(m, adam)
    assert R.same_bits(logits["host"], logits["dev"])
    for name in S.NAMES:
        for slot in snaps["host"][name]:
            assert R.same_bits(snaps["host"][name][slot], snaps["dev"][name][slot]), (name, slot)
