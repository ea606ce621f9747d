"""The WARP reference and its checkers (tests/warp_ref.py, tests/warp_step_ref.py), themselves tested on the CPU: the two
consequences of the contract, the gradients against finite differences of the weighted hinge objective, a float32 NumPy
stand-in for the device (csrc/warp.hip's search, csrc/bpr.hip's hinge form) that passes every check, the same stand-in with
one planted fault rejected, and what the inputs of tests/warp_cases.py reach, from the reference alone."""
import numpy as np
import pytest

from tests import bpr_cases as BC
from tests import bpr_ref as BR
from tests import step_ref as R
from tests import warp_cases as C
from tests import warp_ref as WR
from tests import warp_step_ref as S
from tests.test_bpr_step_ref_host import ALL, _fresh_state, _update
from tests.test_svdpp_step_ref_host import F4, _dot, _finalize, _fma

RND = C.RANDOM[0]


# ----------------------------------------------------------------------------- consequences of the contract
@pytest.mark.parametrize("case", C.RANDOM, ids=lambda c: c["id"])
def test_an_infinite_margin_reproduces_the_bpr_sampler(case):
    w = C.random_world(case)
    neg, trials = WR.search(C.tid_tables(w["t"]), *w["pos"], w["u"], w["i"], float("inf"), seed=C.SEED, step=C.STEP,
                            attempts=1, item_abs=case["item_abs"])
    want = BR.sample(*w["pos"], w["u"], C.R_I, C.SEED, C.STEP, 1)
    assert np.array_equal(neg, want) and (want < 0).any() and (want >= 0).any()
    assert np.array_equal(trials, (want >= 0).astype(np.int64))


def test_a_margin_of_minus_infinity_skips_every_triple():
    w = C.random_world(RND)
    neg, trials = WR.search(C.tid_tables(w["t"]), *w["pos"], w["u"], w["i"], -float("inf"), seed=C.SEED, step=C.STEP)
    assert (neg == -1).all() and (trials == 0).all()


def test_weights():
    assert np.array_equal(WR.weights(200, [0, 1, 2, 100, 199, 200]), [0.0, np.log(199), np.log(99), np.log(1), 0.0, 0.0])
    assert WR.weights(2, [1])[0] == 0.0 and WR.weights(3, [1, 2]).tolist() == [np.log(2), 0.0]


@pytest.mark.parametrize("item_abs,reg_bias", [(False, False), (True, True)])
def test_gradients_are_the_finite_differences_of_the_weighted_hinge(item_abs, reg_bias):
    """with (j, w) held fixed: central differences of ``cost`` at 1e-6 in float64, away from the hinge's kink"""
    rs = np.random.RandomState(3)
    U, I, D, B, lam, margin = 7, 9, 5, 40, 0.03, 0.5
    t = {BR.BI: rs.normal(0, 0.5, I), BR.PF: rs.normal(0, 0.5, (U, D)), BR.QF: rs.normal(0, 0.5, (I, D))}
    u, i, j = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(-1, I, B)
    w = WR.weights(I, rs.randint(1, 5, B))
    x, _, _ = WR.terms(t, u, i, j, w, margin, item_abs, reg_bias)
    assert np.abs(margin - x).min() > 1e-3 and (x < margin).any() and (x >= margin).any() and (j < 0).any()
    G = WR.gradients(t, u, i, j, w, margin, lam, item_abs, reg_bias)
    h = 1e-6
    for k, (g, touched) in G.items():
        num = np.zeros_like(g)
        it = np.nditer(t[k], flags=["multi_index"])
        for _ in it:
            ix = it.multi_index
            keep = t[k][ix]
            t[k][ix] = keep + h
            up = WR.cost(t, u, i, j, w, margin, lam, item_abs, reg_bias)
            t[k][ix] = keep - h
            dn = WR.cost(t, u, i, j, w, margin, lam, item_abs, reg_bias)
            t[k][ix] = keep
            num[ix] = (up - dn) / (2 * h)
        assert np.abs(num - g).max() <= 1e-6 * max(1.0, np.abs(g).max()), k
        assert not g[~touched].any()


# ----------------------------------------------------------------------------- a float32 stand-in for the device
def _device_search(t, pos, u, i, margin, attempts, item_abs, seed, step, fault=None):
    """k_warp_sample in float32: (neg, trials, weights)"""
    indptr, items = pos
    P, Q, bi = (np.asarray(t[k], F4) for k in ("P", "Q", "bi"))
    I = Q.shape[0]
    Qt = np.abs(Q) if item_abs else Q
    c = BR.candidates(seed, step, len(u), I, attempts).astype(np.int64)
    neg, trials = np.full(len(u), -1, np.int64), np.zeros(len(u), np.int64)
    for b, (uu, ii) in enumerate(zip(u, i)):
        row = items[indptr[uu]:indptr[uu + 1]]
        si = _dot(P[uu], Qt[ii]) + bi[ii]
        n = 0
        for cc in c[b]:
            p = np.searchsorted(row, cc)
            positive = p < row.size and row[p] == cc
            if positive and fault != "positives_counted":
                continue
            n += 1
            if positive:
                continue
            x = si - (_dot(P[uu], Qt[cc]) + bi[cc])
            if x < F4(margin):
                neg[b], trials[b] = cc, n
                if fault != "last_violator":
                    break
    return neg, trials


def _device_weights(I, trials, fault=None):
    n = np.asarray(trials, np.int64) + (1 if fault == "weight_of_next_trial" else 0)
    r = np.maximum(1, ((I if fault == "I_for_I_minus_1" else I - 1)) // np.maximum(n, 1))
    return np.where(np.asarray(trials) > 0, np.log(r.astype(F4)), F4(0)).astype(F4)


def _device_step(st, batch, trials, case, s, powers, margin, fault=None):
    """one WARP step in float32 in the kernels' order (k_bpr_users<NJ, true>, k_bpr_items, k_finalize), with the planted
    faults.  Returns (new state, loss, reg)."""
    u, i, j = (np.asarray(a, np.int64) for a in batch)
    if fault == "skipped_touched":
        j = np.where(j < 0, i, j)
    D, frozen = case["D"], case["frozen"]
    lr, lam = BC.hyper_of(case, s)
    lam = F4(lam)
    hyp = dict(opt=case["opt"], lr=F4(lr), alpha=F4(R.alpha_f32(lr, *powers)))
    new = {k: {slot: np.array(a, F4) for slot, a in d.items()} for k, d in st.items()}
    P, Q, bi = (st[k]["w"] for k in ("P", "Q", "bi"))
    wgt = _device_weights(Q.shape[0], np.where(j < 0, 1, trials) if fault == "skipped_touched" else trials, fault)
    item_abs, reg_bias = case["item_abs"], case["reg_bias"]
    B = u.size
    order = np.argsort(u, kind="stable")
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
            wb = wgt[b]
            g = -wb if (x < F4(margin) or fault == "g_not_zeroed") else F4(0)
            if fault == "hinge_sign":
                g = -g
            loss = loss + wb * np.maximum(F4(margin) - x, F4(0))
            rk = (F4(0.5) * psq + F4(0.5) * qisq) + F4(0.5) * qjsq
            if reg_bias:
                rk = rk + (F4(0.5) * (bii * bii) + F4(0.5) * (bij * bij))
            reg = reg + rk
            dp = dp + _fma(g, qi - qj, lam * pu)
            gb[b] = g
            cnt += 1
        scal[p] = (loss, reg, 0)
        if cnt and not frozen >> 3 & 1:
            _update(new, "P", uu, dp, hyp)
    if fault == "items_read_new_P":
        pold = {uu: new["P"]["w"][uu] for uu in pold}
    keys = np.stack((i, np.where(j < 0, i, j)), axis=1).reshape(-1)
    iorder = np.argsort(keys, kind="stable")
    ksi = keys[iorder]
    iheads = np.flatnonzero(np.concatenate(([True], ksi[1:] != ksi[:-1])))
    for p, q in zip(iheads, np.concatenate((iheads[1:], [2 * B]))):
        it = ksi[p]
        qr = Q[it]
        sg = np.sign(qr).astype(F4) if item_abs else np.ones(D, F4)
        dq, dbi, cnt = np.zeros(D, F4), F4(0), 0
        for k in iorder[p:q]:
            b = k >> 1
            if j[b] < 0:
                continue
            g = -gb[b] if k & 1 else gb[b]
            dq = dq + ((g * pold[u[b]]) * sg + lam * qr)
            dbi = dbi + (g + lam * bi[it] if reg_bias else g)
            cnt += 1
        if not cnt:
            continue
        if not frozen >> 4 & 1:
            _update(new, "Q", it, dq, hyp)
        if not frozen >> 2 & 1:
            _update(new, "bi", it, dbi, hyp)
    tot = _finalize(scal)
    return new, tot[0], tot[1]


def _two_device_steps(case, fault=None):
    """two WARP steps of the stand-in on a case of tests/bpr_cases.py, checked as the GPU test checks the device: the
    search (skip cases) against ``check_search``, the step against ``check_warp_step``.  Returns the violated statements."""
    st = _fresh_state(case)
    powers = (R.B1F, R.B2F)
    margin = C.margin_of(case)
    pos = BC.positives(case["kind"])
    bad = []
    for s in range(2):
        u, i, j = BC.batch_of(case, s)
        lr, lam = BC.hyper_of(case, s)
        if case["kind"] == "skip":
            tabs = {k: st[k]["w"] for k in ("P", "Q", "bi")}
            j, trials = _device_search(tabs, pos, u, i, margin, 1, case["item_abs"], BC.SEED, s, fault)
            e = WR.examine(C.tid_tables(tabs), *pos, u, i, margin, seed=BC.SEED, step=s, attempts=1, item_abs=case["item_abs"])
            bad += WR.check_search(e, j, trials)[0]
        else:
            trials = np.ones(u.size, np.int64)
        new, lossv, regv = _device_step(st, (u, i, j), trials, case, s, powers, margin, fault)
        bad += S.check_warp_step(st, new, u, i, j, trials, margin=margin, opt=case["opt"], item_abs=case["item_abs"],
                                 reg_bias=case["reg_bias"], lam=lam, lr=lr, powers=powers, fresh=s == 0, frozen=case["frozen"],
                                 lossv=lossv, regv=regv)
        st, powers = new, (F4(powers[0] * R.B1F), F4(powers[1] * R.B2F))
    return bad


@pytest.mark.parametrize("case", C.STEP_CASES, ids=lambda c: c["id"])
def test_the_device_stand_in_passes_every_check(case):
    bad = _two_device_steps(case)
    assert not bad, bad


def _pick(**kw):
    return [c for c in C.STEP_CASES if all(c[k] == v for k, v in kw.items())][0]


GIVEN_0 = [c for c in C.STEP_CASES if c["kind"] == "edges" and c["opt"] == "adam" and not c["frozen"] and C.margin_of(c) == 0.0][0]
SKIP_CASE = _pick(kind="skip", opt="adam")
STEP_FAULTS = {
    "I_for_I_minus_1": (GIVEN_0, "P"), "weight_of_next_trial": (GIVEN_0, "P"), "hinge_sign": (GIVEN_0, "P"),
    "items_read_new_P": (GIVEN_0, "Q"), "skipped_touched": (SKIP_CASE, "P"), "g_not_zeroed": (GIVEN_0, "P"),
}


@pytest.mark.parametrize("fault", sorted(STEP_FAULTS))
def test_planted_step_faults_are_rejected(fault):
    """Each fault, planted in the stand-in's two steps, is rejected, and a violated statement names the table:

      I_for_I_minus_1       w = log(I / N)                                          P (and Q, bi) gradient
      weight_of_next_trial  w = log((I - 1) / (N + 1))                              P (and Q, bi) gradient
      hinge_sign            g = +w                                                  P (and Q, bi) gradient
      items_read_new_P      the item side reading the updated P                     Q gradient
      skipped_touched       a skipped triple taken with the key it sorts under      P: rows outside the batch changed
      g_not_zeroed          g = -w at x >= margin for a caller's negative           P (and Q, bi) gradient"""
    case, name = STEP_FAULTS[fault]
    assert _two_device_steps(case) == []
    bad = _two_device_steps(case, fault)
    print("fault %s: %d statements violated, first: %s" % (fault, len(bad), bad[:1]))
    assert any(b.startswith(name) for b in bad), "fault %s passes, or no statement names %s: %s" % (fault, name, bad)


@pytest.mark.parametrize("fault,word", [("positives_counted", "N-th open"), ("last_violator", "passed over")])
def test_planted_search_faults_are_rejected(fault, word):
    """positives counted in N; the last violator taken instead of the first: on the random world of GPU test 2"""
    w, e = C.random_world(RND), C.random_reference(RND)
    args = (w["t"], w["pos"], w["u"], w["i"], RND["margin"], RND["attempts"], RND["item_abs"], C.SEED, C.STEP)
    neg, trials = _device_search(*args)
    bad, share = WR.check_search(e, neg, trials)
    assert not bad and share <= C.BAND_CAP, (bad, share)
    neg, trials = _device_search(*args, fault=fault)
    bad, _ = WR.check_search(e, neg, trials)
    print("fault %s: %s" % (fault, bad))
    assert any(word in b for b in bad), bad


# ----------------------------------------------------------------------------- what the inputs reach
@pytest.mark.parametrize("case", C.RANDOM, ids=lambda c: c["id"])
def test_the_random_worlds_keep_the_band_thin(case):
    """the in-band share of GPU test 2's inputs, from the reference alone; if it is higher, change the inputs, not the cap"""
    e = C.random_reference(case)
    share = WR.in_band_share(e)
    print("%s: in-band share %.4f, live %.2f, mean trials %.2f" % (case["id"], share, np.mean(e["neg"] >= 0),
                                                                 e["trials"][e["neg"] >= 0].mean()))
    assert share <= C.BAND_CAP
    assert (e["neg"] >= 0).mean() > 0.5 and (e["trials"] > 1).any()


def test_the_exact_worlds_are_exact_and_reach_what_they_were_built_for():
    ids = {c["id"]: c for c in C.EXACT}
    assert {c["D"] for c in C.EXACT if c["kind"] == "random" and c["I"] == 200} >= set(C.W.BPR)
    assert {c["attempts"] for c in C.EXACT} >= {1, 16, 64} and {c["margin"] for c in C.EXACT} >= {0.0, 1.0, C.INF, -C.INF}
    assert {c["I"] for c in C.EXACT} >= {2, 3, 65, 70000}
    for c in C.EXACT:
        w, e = C.exact_world(c), C.exact_reference(c)
        for k in ("P", "Q", "bi"):
            assert np.array_equal(w["t"][k] * 8, np.round(w["t"][k] * 8)) and np.abs(w["t"][k]).max() <= 2
        assert w["u"].size % 4 != 0
        if c["kind"] == "random":
            lens = np.diff(w["pos"][0])
            assert set(C.ROW_LENGTHS) & set(range(c["I"] + 1)) <= set(lens.tolist()) and {c["I"], c["I"] - 1} <= set(lens.tolist())
            full = int(np.flatnonzero(lens == c["I"])[0])
            assert (e["neg"][w["u"] == full] == -1).all()
    for a in (16, 64):                                     # the planted worlds: a violator at every candidate position
        c = ids["planted-D16-I70000-a%d-m1.0" % a]
        e = C.exact_reference(c)
        live = e["neg"] >= 0
        at = np.argmax(e["open"] & (e["n"] == e["trials"][:, None]), 1)[live]
        assert set(at.tolist()) >= {0, a - 1} | set(range(2, C.GROUP + 2)), sorted(set(at.tolist()))
        assert len(set(at.tolist())) >= a - a // 8         # (two triples' candidates may collide: nearly every position)
        assert set(e["trials"][live].tolist()) >= set(range(1, C.GROUP + 3))       # every slot of a load group, and past it
        assert (e["trials"][live] < at + 1).any()                                   # positives before the violator
        assert len(set(e["trials"][live].tolist())) >= a // 2                        # many distinct weights
    for name, i_num in (("planted_rows-D3-I2-a16-m1.0", 2), ("planted_rows-D4-I3-a16-m1.0", 3), ("planted_rows-D68-I65-a64-m1.0", 65)):
        e = C.exact_reference(ids[name])                   # (I - 1) // N reaches 1: the weight 0, next to weights above it
        wl = WR.weights(i_num, e["trials"][e["neg"] >= 0])
        assert (wl == 0).any() and ((wl > 0).any() or i_num == 2), name
    e = C.exact_reference(ids["random-D33-I200-a16-minf"])
    w = C.exact_world(ids["random-D33-I200-a16-minf"])
    assert np.array_equal(e["neg"], BR.sample(*w["pos"], w["u"], 200, C.SEED, C.STEP, 16))
    assert (C.exact_reference(ids["random-D33-I200-a16-m-inf"])["neg"] == -1).all()
