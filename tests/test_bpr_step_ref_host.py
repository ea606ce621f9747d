"""The per-row BPR step checks of tests/bpr_step_ref.py, themselves tested on the CPU: the float64 sums agree with
tests/bpr_ref.py, the float32 restatement stays inside the bound on every case of tests/bpr_cases.py, a float32 NumPy
stand-in for the device (csrc/bpr.hip's order of operations) passes every check on every case, and the same stand-in with
one planted fault is rejected by a statement that names the table."""
import time

import numpy as np
import pytest

from oracle import svd_oracle as so
from tests import bpr_cases as C
from tests import bpr_ref as BR
from tests import bpr_step_ref as S
from tests import step_ref as R
from tests.test_svdpp_step_ref_host import F4, _dot, _finalize, _fma

ALL = ("mu", "bu", "bi", "P", "Q")


# ----------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_the_float64_sums_are_the_contracts(case):
    t = C.tables_of(case)
    t64 = {S.TID[k]: np.asarray(t[k], np.float64) for k in ALL}
    for s in range(2):
        u, i, j = C.batch_of(case, s)
        lam = C.hyper_of(case, s)[1]
        t0 = time.time()
        ref, terms = S.bpr_step_grads(t, u, i, j, case["item_abs"], case["reg_bias"], lam)
        print("TIME %s step%d float64 reference %.2f s" % (case["id"], s, time.time() - t0))
        G = BR.gradients(t64, u, i, j, lam, case["item_abs"], case["reg_bias"])
        for name in S.NAMES:
            g, touched = G[S.TID[name]]
            assert np.abs(ref[name][0] - g).max() <= 1e-12 * max(1.0, float(np.abs(g).max())), name
            assert np.array_equal(np.reshape(ref[name][2], (-1,)) > 0, touched), name
        x, data, reg = BR.terms(t64, u, i, j, case["item_abs"], case["reg_bias"])
        assert np.abs(terms["x"] - x).max() <= 1e-12 * max(1.0, np.abs(x).max())
        assert abs(terms["loss"][0] - data) <= 1e-12 * max(1.0, data) and abs(terms["reg"][0] - reg) <= 1e-12 * max(1.0, reg)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_float32_restatement_stays_inside_the_bound(case):
    t = C.tables_of(case)
    for s in range(2):
        u, i, j = C.batch_of(case, s)
        lam = C.hyper_of(case, s)[1]
        ref, terms = S.bpr_step_grads(t, u, i, j, case["item_abs"], case["reg_bias"], lam)
        f32 = S.f32_bpr(t, u, i, j, case["item_abs"], case["reg_bias"], lam)
        ref = dict(ref, loss=terms["loss"], reg=terms["reg"])
        for name in S.NAMES + ("loss", "reg"):
            G, E, n = (np.atleast_1d(a) for a in ref[name])
            c = R.ratio(np.atleast_1d(f32[name]), G, E, n)
            print("%s step%d %s: c_ref short %.2f long %.2f (longest run %d)" % (case["id"], s, name, c["short"], c["long"], int(np.max(n))))
            assert np.isfinite(list(c.values())).all() and c["short"] <= R.LONG_RUN and c["long"] <= max(1, np.max(n)), (name, c)


# ----------------------------------------------------------------------------- a float32 stand-in for the device
def _update(st, name, idx, g, hyp, fault=None):
    """bpr_update on the elements ``idx`` of a table"""
    w, g = st[name]["w"], np.asarray(g, F4)
    if hyp["opt"] == "sgd":
        w[idx] = w[idx] - hyp["lr"] * g
        return
    m, v = st[name]["m"], st[name]["v"]
    omb1, omb2 = F4(1) - R.B1F, F4(1) - R.B2F
    mm = _fma(m[idx], R.B1F, g * omb1)
    vv = _fma(v[idx], R.B2F, (g * g) * omb2 if fault != "v_no_factor:" + name else g * g)
    m[idx], v[idx] = mm, vv
    step = hyp["lr"] if fault == "lr_for_alpha:" + name else hyp["alpha"]
    w[idx] = w[idx] - step * mm / (np.sqrt(vv) + F4(so.EPSILON))


def _device_step(st, batch, case, s, powers, fault=None):
    """one step in float32 in the kernels' order (k_bpr_users, k_bpr_items, k_finalize), with the planted faults.
    Returns (new state, loss, reg)."""
    u, i, j = (np.asarray(a, np.int64) for a in batch)
    if fault == "skipped_counted":                        # a skipped triple taken with the key it sorts under
        j = np.where(j < 0, i, j)
    D, frozen = case["D"], case["frozen"]
    lr, lam = C.hyper_of(case, s)
    lam = F4(lam)
    hyp = dict(opt=case["opt"], lr=F4(lr), alpha=F4(R.alpha_f32(lr, *powers)))
    new = {k: {slot: np.array(a, F4) for slot, a in d.items()} for k, d in st.items()}
    P, Q, bi = (st[k]["w"] for k in ("P", "Q", "bi"))
    item_abs, reg_bias = case["item_abs"], case["reg_bias"]
    B = u.size
    order = np.argsort(u, kind="stable")                  # triples by user, batch order within a run
    ks = u[order]
    heads = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1])))
    scal = np.zeros((B, 3), F4)
    gb, pold = np.zeros(B, F4), {}
    for p, q in zip(heads, np.concatenate((heads[1:], [B]))):
        uu = ks[p]
        pu = P[uu].copy()
        pold[uu] = pu
        psq = _dot(pu, pu)
        dp, loss, reg, cnt = np.zeros(D, F4), F4(0), F4(0), 0
        for b in order[p:q]:
            if j[b] < 0:
                continue
            x1, x2 = Q[i[b]], Q[j[b]]
            qi, qj = (np.abs(x1), np.abs(x2)) if item_abs else (x1, x2)
            di, dj, qisq, qjsq = _dot(pu, qi), _dot(pu, qj), _dot(x1, x1), _dot(x2, x2)
            bii, bij = bi[i[b]], bi[j[b]]
            x = (di + bii) - (dj + bij)
            g = F4(-1) / (F4(1) + np.exp(x))
            loss = loss + (np.maximum(-x, F4(0)) + np.log1p(np.exp(-np.abs(x))))
            rk = (F4(0.5) * psq + F4(0.5) * qisq) + F4(0.5) * qjsq
            if reg_bias:
                rk = rk + (F4(0.5) * (bii * bii) + F4(0.5) * (bij * bij))
            reg = reg + rk
            dp = dp + _fma(g, qi - qj, lam * pu)
            gb[b] = g
            cnt += 1
        scal[p] = (loss, reg, 0)
        if cnt and not frozen >> 3 & 1:
            _update(new, "P", uu, dp, hyp, fault)
        elif cnt and fault == "frozen_m:P":
            new["P"]["m"][uu] = _fma(new["P"]["m"][uu], R.B1F, dp * (F4(1) - R.B1F))
    if fault == "items_read_new_P":
        pold = {uu: new["P"]["w"][uu] for uu in pold}
    # the 2B occurrences by item: key 2b the positive, 2b + 1 the negative (a skipped triple's sorts with its positive)
    keys = np.stack((i, np.where(j < 0, i, j)), axis=1).reshape(-1)
    iorder = np.argsort(keys, kind="stable")
    ksi = keys[iorder]
    iheads = np.flatnonzero(np.concatenate(([True], ksi[1:] != ksi[:-1])))
    for p, q in zip(iheads, np.concatenate((iheads[1:], [2 * B]))):
        it = ksi[p]
        qr = Q[it]
        sg = np.sign(qr).astype(F4) if item_abs else np.ones(D, F4)
        if fault == "sign0_is_1" and item_abs:
            sg = np.where(qr == 0, F4(1), sg)
        dq, dbi, cnt = np.zeros(D, F4), F4(0), 0
        for k in iorder[p:q]:
            b = k >> 1
            if j[b] < 0:
                continue
            g = -gb[b] if (k & 1) and fault != "neg_sign_lost" else gb[b]
            dq = dq + ((g * pold[u[b]]) * sg + lam * qr)
            dbi = dbi + (g + lam * bi[it] if reg_bias else g)
            cnt += 1
        if not cnt:
            continue
        if not frozen >> 4 & 1:
            _update(new, "Q", it, dq, hyp, fault)
        if not frozen >> 2 & 1:
            _update(new, "bi", it, dbi, hyp, fault)
    tot = _finalize(scal)
    return new, tot[0], tot[1]


def _fresh_state(case):
    t = C.tables_of(case)
    st = {k: dict(w=np.array(t[k], F4)) for k in ALL}
    if case["opt"] == "adam":
        for k in ALL:
            st[k].update(m=np.zeros(np.shape(t[k]), F4), v=np.zeros(np.shape(t[k]), F4))
    return st


def _two_device_steps(case, fault=None):
    st = _fresh_state(case)
    powers = (R.B1F, R.B2F)
    bad = []
    for s in range(2):
        u, i, j = C.batch_of(case, s)
        lr, lam = C.hyper_of(case, s)
        new, lossv, regv = _device_step(st, (u, i, j), case, s, powers, fault)
        bad += S.check_bpr_step(st, new, u, i, j, opt=case["opt"], item_abs=case["item_abs"], reg_bias=case["reg_bias"], lam=lam,
                                lr=lr, powers=powers, fresh=s == 0, frozen=case["frozen"], lossv=lossv, regv=regv)
        st, powers = new, (F4(powers[0] * R.B1F), F4(powers[1] * R.B2F))
    return bad


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_the_device_stand_in_passes_every_check(case):
    bad = _two_device_steps(case)
    assert not bad, bad


def _pick(**kw):
    return [c for c in C.CASES if all(c[k] == v for k, v in kw.items())][0]


ADAM_CASE = _pick(kind="edges", opt="adam", item_abs=True, frozen=0, hyper2=None)
SKIP_CASE = _pick(kind="skip", opt="adam")
FROZEN_P = _pick(frozen=1 << BR.PF)
# fault -> (case, what a violated statement must start with)
FAULTS = {
    "items_read_new_P": (ADAM_CASE, "Q"), "sign0_is_1": (ADAM_CASE, "Q"), "neg_sign_lost": (ADAM_CASE, "Q"),
    "skipped_counted": (SKIP_CASE, "P"), "v_no_factor:Q": (ADAM_CASE, "Q: v"), "v_no_factor:P": (ADAM_CASE, "P: v"),
    "lr_for_alpha:bi": (ADAM_CASE, "bi: w"), "lr_for_alpha:P": (ADAM_CASE, "P: w"), "frozen_m:P": (FROZEN_P, "P.m"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_faults_are_rejected(fault):
    """Each fault, planted in the stand-in's two steps, is rejected, and a violated statement names the table:

      items_read_new_P  the item side reading the updated P                        Q gradient
      sign0_is_1        sign(0) taken as 1 under item_abs                          Q gradient
      neg_sign_lost     the negative role's -g taken as +g                         Q (and bi) gradient
      skipped_counted   a skipped triple counted                                   P (and Q, bi): rows outside the batch changed
      v_no_factor       v built from g g without (1 - b2)                          v does not follow from g
      lr_for_alpha      the apply using lr where alpha belongs                     w does not follow from m and v
      frozen_m          a frozen table's m advanced                                P.m: a frozen table changed"""
    case, name = FAULTS[fault]
    assert _two_device_steps(case) == []
    bad = _two_device_steps(case, fault)
    print("fault %s: %d statements violated, first: %s" % (fault, len(bad), bad[:1]))
    assert any(b.startswith(name) for b in bad), "fault %s passes, or no statement names %s: %s" % (fault, name, bad)


def test_cases_cover_what_the_kernels_are_built_around():
    from tests import widths as W
    edges = [c for c in C.CASES if c["kind"] == "edges"]
    assert {c["D"] for c in edges} >= set(W.BPR)
    assert {c["tail"] for c in edges} >= {33, 65}
    assert {c["frozen"] for c in C.CASES if c["opt"] == "adam"} >= {1 << BR.BI, 1 << BR.PF, 1 << BR.QF}
    assert {c["opt"] for c in C.CASES if c["kind"] == "skip"} == {"adam", "sgd"}
    assert any(c["hyper2"] for c in C.CASES) and any(c["item_abs"] for c in edges)
    for key in ("item_abs", "reg_bias", "opt"):
        assert len({c[key] for c in edges}) == 2, key
