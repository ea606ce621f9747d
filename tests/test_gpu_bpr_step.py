"""The BPR training step, per row: the gradient sum the device used for P, Q and bi over the live triples, its Adam moments
and its apply, each held to its own statement (tests/bpr_step_ref.py), its data loss and its regulariser; mu, bu and
every row no live triple names hold their bits in every slot.  Two successive steps on a fresh model; every table and its
m and v are read before, between and after.  The cases are tests/bpr_cases.py: every run edge of csrc/bpr.hip, the hazard
chain, j == i, skipped triples, sign(0), frozen tables."""
import time

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import bpr_cases as C
from tests import bpr_step_ref as S
from tests import step_ref as R
from tests import widths as W

pytestmark = pytest.mark.gpu

ALL = ("mu", "bu", "bi", "P", "Q")
assert {c["D"] for c in C.CASES if c["kind"] == "edges"} >= set(W.BPR)


def _snapshot(m, adam):
    out = {}
    for name in ALL:
        tid = S.TID[name]
        d = dict(w=m.get_table(tid))
        if adam:
            d["m"], d["v"] = m.get_table(tid | L.SLOT_M), m.get_table(tid | L.SLOT_V)
        out[name] = d
    return out


def _model(case):
    lr, lam = C.hyper_of(case, 0)
    t = C.tables_of(case)
    m = T.SvdModel(case["U"], case["I"], case["D"], item_abs=case["item_abs"], reg_bias=case["reg_bias"], optimizer=case["opt"],
                   adam_mode="lazy", lr=lr, reg=lam)
    m.set_tables(*(t[k] for k in ALL))
    m.set_positives(C.positives(case["kind"]))
    if case["kind"] == "skip":
        m.set_bpr_sampler(C.SEED, 1)
    if case["frozen"]:
        m.set_frozen(case["frozen"])
    return m


def _check_two_steps(case, report):
    adam = case["opt"] == "adam"
    with _model(case) as m:
        assert m.get_step()[0] == 0
        before = _snapshot(m, adam)
        for s in range(2):
            if s == 1 and case["hyper2"]:
                m.set_hyper(*case["hyper2"])
            lr, lam = C.hyper_of(case, s)
            u, i, j = C.batch_of(case, s)
            _, b1p, b2p = m.get_step()
            sampled = case["kind"] == "skip"
            neg, lossv, regv, skipped = m.train_bpr_step(u, i, None if sampled else j)
            after = _snapshot(m, adam)
            assert m.get_step()[0] == s + 1
            assert np.array_equal(neg, j) and skipped == (int(np.sum(j < 0)) if sampled else 0)
            rep = report.setdefault("step%d" % s, {})
            t0 = time.time()
            bad = S.check_bpr_step(before, after, u, i, j, opt=case["opt"], item_abs=case["item_abs"], reg_bias=case["reg_bias"],
                                   lam=lam, lr=lr, powers=(b1p, b2p), fresh=s == 0, frozen=case["frozen"], lossv=lossv, regv=regv,
                                   report=rep)
            print("TIME %s step%d NumPy reference and checks %.1f s" % (case["id"], s, time.time() - t0))
            assert not bad, "%s, step %d:\n  %s" % (case["id"], s, "\n  ".join(bad))
            before = after


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_two_bpr_steps_per_row(case):
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


@pytest.mark.parametrize("case", [c for c in C.CASES if c["tail"] == 65 or c["kind"] == "skip" and c["opt"] == "adam"],
                         ids=lambda c: c["id"])
def test_train_bpr_step_dev_equals_train_bpr_step_bit_for_bit(case):
    """tfr_bpr_train_step_dev on device columns, given and sampled negatives: the negatives it reports, every table and
    every slot equal those of tfr_bpr_train_step on the same host columns"""
    torch = pytest.importorskip("torch")
    adam = case["opt"] == "adam"
    sampled = case["kind"] == "skip"
    snaps, negs = {}, {}
    for how in ("host", "dev"):
        with _model(case) as m:
            for s in range(2):
                u, i, j = C.batch_of(case, s)
                if how == "host":
                    negs[how, s] = m.train_bpr_step(u, i, None if sampled else j)[0]
                    continue
                d = [torch.from_numpy(a).cuda() for a in (u, i, j)]
                out = m.train_bpr_step_dev(d[0], d[1], None if sampled else d[2], want_negatives=True)
                m.sync()
                torch.cuda.synchronize()
                negs[how, s] = out.cpu().numpy()
            assert m.get_step()[0] == 2
            snaps[how] = _snapshot(m, adam)
    for s in range(2):
        assert np.array_equal(negs["host", s], negs["dev", s])
    for name in ALL:
        for slot in snaps["host"][name]:
            assert R.same_bits(snaps["host"][name][slot], snaps["dev"][name][slot]), (name, slot)
