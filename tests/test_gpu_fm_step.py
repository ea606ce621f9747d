"""The FM training step, per row: the gradient sum the device used for V, W and mu, its Adam moments and its apply, each held
to its own statement (tests/fm_ref.py), the step's predictions per row and its data loss.  Two successive steps on a fresh
model; mu, W, V and their m and v are read before, between and after.  The cases are tests/fm_cases.py."""
import time

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import fm_cases as C
from tests import fm_ref as FR
from tests import step_ref as R
from tests import widths as W

pytestmark = pytest.mark.gpu

assert {c["D"] for c in C.CASES if c["kind"] == "edges"} >= set(W.FM_STEP)


def _snapshot(m, adam):
    out = {}
    for name in FR.NAMES:
        tid = FR.TID[name]
        d = dict(w=m.get_table(tid))
        if adam:
            d["m"], d["v"] = m.get_table(tid | L.SLOT_M), m.get_table(tid | L.SLOT_V)
        out[name] = d
    return out


def _model(case):
    lr, lam = C.hyper_of(case)
    return T.FmModel(case["F"], case["D"], loss=case["loss"], optimizer=case["opt"], lr=lr, reg=lam)


def _check_two_steps(case, report):
    adam = case["opt"] == "adam"
    lr, lam = C.hyper_of(case)
    t = C.tables_of(case)
    with _model(case) as m:
        m.set(t["mu"], t["W"], t["V"])
        assert m.get_step()[0] == 0
        before = _snapshot(m, adam)
        for s in range(2):
            csr, y = C.batch_of(case, s)
            _, b1p, b2p = m.get_step()
            pred, lossv = m.train_step(C.as_csr(csr, case["F"]), y)
            after = _snapshot(m, adam)
            assert m.get_step()[0] == s + 1
            rep = report.setdefault("step%d" % s, {})
            bad = FR.check_fm_step(before, after, csr, y, opt=case["opt"], loss=case["loss"], lam=lam, lr=lr, powers=(b1p, b2p),
                                   fresh=s == 0, pred=pred, lossv=lossv, report=rep)
            assert not bad, "%s, step %d:\n  %s" % (case["id"], s, "\n  ".join(bad))
            if case["kind"] == "empty":                   # no entries: V, W and their slots keep their bits, mu moves
                for name in ("V", "W"):
                    for slot in before[name]:
                        assert R.same_bits(before[name][slot], after[name][slot]), (name, slot)
                assert not R.same_bits(before["mu"]["w"], after["mu"]["w"])
                assert np.all(pred == before["mu"]["w"])
            before = after


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_two_fm_steps_per_row(case):
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


# ----------------------------------------------------------------------------- the device entry points
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("case", [c for c in C.CASES if c["id"] in ("edges-F400-D64-n701-nll_adam", "edges-F400-D100-n701-mse_sgd")],
                         ids=lambda c: c["id"])
def test_train_step_dev_equals_train_step_bit_for_bit(case):
    """tfr_fm_train_step_dev on device CSR arrays, first without a prediction buffer (the training forward then has no `out`),
    then with one: tables, slots and predictions equal those of tfr_fm_train_step on the same host arrays"""
    torch = pytest.importorskip("torch")
    adam = case["opt"] == "adam"
    t = C.tables_of(case)
    snaps, preds = {}, {}
    for how in ("host", "dev"):
        with _model(case) as m:
            m.set(t["mu"], t["W"], t["V"])
            for s in range(2):
                (indptr, indices, data), y = C.batch_of(case, s)
                if how == "host":
                    preds[how, s] = m.train_step(C.as_csr((indptr, indices, data), case["F"]), y)[0]
                    continue
                d = [_dev(torch, a) for a in (indptr, indices, data, y)]
                out = torch.full((y.size,), float("nan"), dtype=torch.float32, device="cuda") if s == 1 else None
                torch.cuda.synchronize()
                m.train_step_dev(*(a.data_ptr() for a in d), y.size, indices.size, out.data_ptr() if s == 1 else None)
                m.sync()
                torch.cuda.synchronize()
                preds[how, s] = out.cpu().numpy() if s == 1 else None
            assert m.get_step()[0] == 2
            snaps[how] = _snapshot(m, adam)
    assert np.array_equal(preds["host", 1].view(np.uint32), preds["dev", 1].view(np.uint32))
    for name in FR.NAMES:
        for slot in snaps["host"][name]:
            assert R.same_bits(snaps["host"][name][slot], snaps["dev"][name][slot]), (name, slot)


def test_forward_dev_equals_forward_csr_bit_for_bit():
    torch = pytest.importorskip("torch")
    case = [c for c in C.CASES if c["id"] == "edges-F400-D100-n701-nll_adam"][0]
    t = C.tables_of(case)
    (indptr, indices, data), _ = C.batch_of(case, 0)
    with _model(case) as m:
        m.set(t["mu"], t["W"], t["V"])
        want = m.forward_csr(indptr, indices, data)
        d = [_dev(torch, a) for a in (indptr, indices, data)]
        out = torch.full((indptr.size - 1,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        m.forward_dev(*(a.data_ptr() for a in d), indptr.size - 1, out.data_ptr())
        m.sync()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not FR.forward_excess(got, t["mu"], t["W"], t["V"], indptr, indices, data)
