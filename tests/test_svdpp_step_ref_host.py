"""The per-row SVD++ step checks of tests/svdpp_step_ref.py, themselves tested on the CPU: the float64 sums agree with
tests/svdpp_ref.py, the float32 restatement stays inside the bound on every case of tests/svdpp_cases.py, a float32 NumPy
stand-in for the device (csrc/svdpp.hip's order of operations) passes every check on every case, and the same stand-in with
one planted fault is rejected by a statement that names the table."""
import time

import numpy as np
import pytest

from oracle import svd_oracle as so
from tests import step_ref as R
from tests import svdpp_cases as C
from tests import svdpp_ref as PR
from tests import svdpp_step_ref as S

F4 = np.float32
FLAGS = lambda c: (c["loss"], c["item_abs"], c["reg_bias"])


# ----------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_the_float64_sums_are_the_contracts(case):
    t, N = C.tables_of(case), C.implicit()
    for s in range(2):
        u, i, r = C.batch_of(case, s)
        lam = C.hyper_of(case, s)[1]
        t0 = time.time()
        ref, terms = S.svdpp_step_grads(t, *N, u, i, r, *FLAGS(case), lam)
        print("TIME %s step%d float64 reference %.2f s" % (case["id"], s, time.time() - t0))
        t64 = S.by_id(t, np.float64)
        G = PR.gradients(t64, N[0], N[1], u.astype(np.int64), i.astype(np.int64), r.astype(np.float64), *FLAGS(case), lam)
        for name in S.NAMES:
            scale = max(1.0, float(np.abs(G[S.TID[name]]).max()))
            assert np.abs(ref[name][0] - G[S.TID[name]]).max() <= 1e-12 * scale, name
        x = PR.forward(t64, N[0], N[1], u.astype(np.int64), i.astype(np.int64), case["item_abs"])
        assert np.abs(terms["x"] - x).max() <= 1e-12 * max(1.0, np.abs(x).max())
        lossv, regv = so.data_loss(x, r.astype(np.float64), case["loss"]), PR.regularizer(t64, N[0], N[1], u, i, case["reg_bias"])
        assert abs(terms["loss"][0] - lossv) <= 1e-12 * max(1.0, abs(lossv)) and abs(terms["reg"][0] - regv) <= 1e-12 * max(1.0, regv)
        assert np.array_equal(ref["Y"][2][:, 0] > 0, S.touched_y(N[0], N[1], u, C.I))


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_float32_restatement_stays_inside_the_bound(case):
    """a sequential float32 sum of n terms is off by at most n eps32 sum |terms| beyond E, so c_ref is finite and at most
    LONG_RUN for the short class, the longest run for the long one"""
    t, N = C.tables_of(case), C.implicit()
    for s in range(2):
        u, i, r = C.batch_of(case, s)
        lam = C.hyper_of(case, s)[1]
        ref, terms = S.svdpp_step_grads(t, *N, u, i, r, *FLAGS(case), lam)
        f32 = S.f32_svdpp(t, *N, u, i, r, *FLAGS(case), lam)
        ref = dict(ref, x=(terms["x"], terms["X"], terms["nN"]), loss=terms["loss"], reg=terms["reg"])
        for name in S.NAMES + ("x", "loss", "reg"):
            G, E, n = (np.atleast_1d(a) for a in ref[name])
            c = R.ratio(np.atleast_1d(f32[name]), G, E, n)
            print("%s step%d %s: c_ref short %.2f long %.2f (longest run %d)" % (case["id"], s, name, c["short"], c["long"], int(np.max(n))))
            assert np.isfinite(list(c.values())).all() and c["short"] <= R.LONG_RUN and c["long"] <= max(1, np.max(n)), (name, c)


# ----------------------------------------------------------------------------- a float32 stand-in for the device
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F4)


def _lanes(a):
    """[..., D] -> [..., NJ, 64]: feature f = lane + 64 j, zero beyond D"""
    D = a.shape[-1]
    nj = -(-D // 64)
    out = np.zeros(a.shape[:-1] + (nj * 64,), F4)
    out[..., :D] = a
    return out.reshape(a.shape[:-1] + (nj, 64))


def _butterfly(v):
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def _dot(a, b):
    """wave_sum_all (csrc/wave_rows.h) of a per-lane fmaf chain over j"""
    A, B = _lanes(a), _lanes(b)
    acc = np.zeros(A.shape[:-2] + (64,), F4)
    for j in range(A.shape[-2]):
        acc = _fma(A[..., j, :], B[..., j, :], acc)
    return _butterfly(acc)


def _seq(rows):
    """a float32 sum of rows in order, from zero"""
    rows = np.asarray(rows, F4)
    return np.cumsum(rows, axis=0, dtype=F4)[-1] if rows.shape[0] else np.zeros(rows.shape[1:], F4)


def _update(st, name, idx, g, hyp, fault=None):
    """pp_update on the elements ``idx`` of a table (finalize.inc.h's dense form for mu)"""
    w, g = st[name]["w"], np.asarray(g, F4)
    if hyp["opt"] == "sgd":
        w[idx] = w[idx] - hyp["lr"] * g
        return
    m, v = st[name]["m"], st[name]["v"]
    omb1, omb2 = F4(1) - R.B1F, F4(1) - R.B2F
    if name == "mu":
        mm = _fma(g - m[idx], omb1, m[idx])
        vv = _fma(g * g - v[idx], omb2, v[idx])
    else:
        mm = _fma(m[idx], R.B1F, g * omb1)
        vv = _fma(v[idx], R.B2F, (g * g) * omb2 if fault != "v_no_factor:" + name else g * g)
    m[idx], v[idx] = mm, vv
    step = hyp["lr"] if fault == "lr_for_alpha:" + name else hyp["alpha"]
    w[idx] = w[idx] - (step * mm) / (np.sqrt(vv) + F4(so.EPSILON))
    return


def _finalize(scal):
    """k_finalize's fixed order over the per-position partials: thread t adds positions t, t + 256, ...; a wave's 64 sums
    by shfl_down halving; (w0 + w1) + (w2 + w3)"""
    n = scal.shape[0]
    pad = np.zeros((-(-max(n, 1) // 256) * 256,) + scal.shape[1:], F4)
    pad[:n] = scal
    acc = np.cumsum(pad.reshape(-1, 256, scal.shape[1]), axis=0, dtype=F4)[-1].reshape(4, 64, -1)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc[:, :o] + acc[:, o:2 * o]
    w = acc[:, 0]
    return (w[0] + w[1]) + (w[2] + w[3])


def _device_step(st, N, batch, case, s, powers, fault=None):
    """one step in float32 in the kernels' order (k_pp_ypart, k_pp_users, k_pp_items, k_pp_ygrad, k_pp_yapply, k_finalize),
    with the planted faults.  Returns (new state, logits, loss, reg)."""
    indptr, items = N
    u, i, r = batch
    D, frozen = case["D"], case["frozen"]
    lr, lam = C.hyper_of(case, s)
    lam = F4(lam)
    hyp = dict(opt=case["opt"], lr=F4(lr), alpha=F4(R.alpha_f32(lr, *powers)))
    new = {k: {slot: np.array(a, F4) for slot, a in d.items()} for k, d in st.items()}
    P, Q, bu, bi, Y = (st[k]["w"] for k in ("P", "Q", "bu", "bi", "Y"))
    mu = F4(st["mu"]["w"])
    item_abs, reg_bias, mse = case["item_abs"], case["reg_bias"], case["loss"] == "mse"
    B = u.size
    order = np.argsort(u, kind="stable")
    ks = u[order]
    heads = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1])))
    ends = np.concatenate((heads[1:], [B]))
    # k_pp_ypart: per piece of N of an active user, its Y rows ascending
    parts, psq_parts = {}, {}
    for uu in ks[heads]:
        js = items[indptr[uu]:indptr[uu + 1]]
        parts[uu], psq_parts[uu] = [], []
        for a in range(0, js.size, C.PIECE):
            pj = js[a:a + C.PIECE]
            if fault == "z_last" and pj.size > 1:
                pj = pj[:-1]
            rows = Y[pj]
            parts[uu].append(_seq(rows))
            L = _lanes(rows)
            acc = np.zeros(64, F4)
            for row in L:
                for lj in row:
                    acc = _fma(lj, lj, acc)
            psq_parts[uu].append(_butterfly(acc))
    active = list(ks[heads])
    peff, W, cnt, sfac, zs = {}, {}, {}, {}, {}
    scal = np.zeros((B, 3), F4)
    logits, gk = np.zeros(B, F4), np.zeros(B, F4)
    for x, (p, q) in enumerate(zip(heads, ends)):
        uu = ks[p]
        mine = list(parts[uu])
        if fault == "neighbour_part" and mine:            # the last piece's partial is the next active user's first
            nxt = [v for v in active[x + 1:] + active[:x] if parts[v]]
            mine[-1] = parts[nxt[0]][0]
        z = _seq(mine) if mine else np.zeros(D, F4)
        ysq = _seq(psq_parts[uu]) if mine else F4(0)
        nu = indptr[uu + 1] - indptr[uu]
        sv = F4(1) / np.sqrt(F4(nu)) if nu > 0 else F4(0)
        pu = P[uu]
        pe = _fma(sv, z, pu)
        peff[uu], sfac[uu], zs[uu] = pe, sv, z
        psq = _dot(pu, pu)
        e = order[p:q]
        qq = Q[i[e]]
        qt = np.abs(qq) if item_abs else qq
        xs = ((_dot(np.broadcast_to(pe, qt.shape), qt) + mu) + bu[uu]) + bi[i[e]]
        qsq = _dot(qq, qq)
        rt = r[e]
        if mse:
            g = xs - rt
            lk = F4(0.5) * (g * g)
        else:
            g = (F4(1) / (F4(1) + np.exp(-xs)) - rt).astype(F4)
            lk = (np.maximum(xs, F4(0)) - xs * rt + np.log1p(np.exp(-np.abs(xs)))).astype(F4)
        logits[e], gk[e] = xs, g
        wacc, dp = np.zeros(D, F4), np.zeros(D, F4)
        loss = reg = sumg = dbu = F4(0)
        for k in range(e.size):
            wacc = _fma(g[k], qt[k], wacc)
            dp = dp + _fma(g[k], qt[k], lam * pu)
            rk = F4(0.5) * psq + F4(0.5) * qsq[k]
            if reg_bias:
                rk = rk + (F4(0.5) * (bu[uu] * bu[uu]) + F4(0.5) * (bi[i[e[k]]] * bi[i[e[k]]]))
                dbu = dbu + (g[k] + lam * bu[uu])
            else:
                dbu = dbu + g[k]
            reg = reg + (rk + F4(0.5) * ysq if fault != "no_ysq" else rk)
            loss, sumg = loss + lk[k], sumg + g[k]
        W[uu] = sv * wacc if fault != "no_s_in_W" else wacc
        cnt[uu] = e.size if fault != "c_one" else 1
        scal[p] = (loss, reg, sumg)
        if not frozen >> 3 & 1:
            _update(new, "P", uu, dp, hyp, fault)
        elif fault == "frozen_m:P":
            new["P"]["m"][uu] = _fma(new["P"]["m"][uu], R.B1F, dp * (F4(1) - R.B1F))
        if not frozen >> 1 & 1:
            _update(new, "bu", uu, dbu, hyp, fault)
    # k_pp_items: per item run in batch order, from peff and g of the tables before the step
    if fault == "items_read_new_P":
        peff = {uu: _fma(sfac[uu], zs[uu], new["P"]["w"][uu]) for uu in peff}
    iorder = np.argsort(i, kind="stable")
    ksi = i[iorder]
    iheads = np.flatnonzero(np.concatenate(([True], ksi[1:] != ksi[:-1])))
    for p, q in zip(iheads, np.concatenate((iheads[1:], [B]))):
        it = ksi[p]
        qr = Q[it]
        sg = np.sign(qr).astype(F4) if item_abs else np.ones(D, F4)
        if fault == "sign0_is_1" and item_abs:
            sg = np.where(qr == 0, F4(1), sg)
        dq, dbi = np.zeros(D, F4), F4(0)
        for k in iorder[p:q]:
            dq = dq + ((gk[k] * peff[u[k]]) * sg + lam * qr)
            dbi = dbi + (gk[k] + lam * bi[it] if reg_bias else gk[k])
        if not frozen >> 4 & 1:
            _update(new, "Q", it, dq, hyp, fault)
        elif fault == "frozen_m:Q":
            new["Q"]["m"][it] = _fma(new["Q"]["m"][it], R.B1F, dq * (F4(1) - R.B1F))
        if not frozen >> 2 & 1:
            _update(new, "bi", it, dbi, hyp, fault)
    # k_pp_ygrad / k_pp_yapply: per piece of NT its active users ascending; per Y row its pieces in order
    if not frozen >> 5 & 1:
        tip, tusers = C.transpose(indptr, items)
        for j in range(Y.shape[0]):
            col = tusers[tip[j]:tip[j + 1]]
            gy, c = np.zeros(D, F4), 0
            for a in range(0, col.size, C.PIECE):
                acc, cc = np.zeros(D, F4), 0
                for uu in col[a:a + C.PIECE]:
                    if uu in W:
                        lc = lam * F4(cnt[uu])
                        acc = acc + (_fma(lc, Y[j], W[uu]) if fault != "no_lamcY" else W[uu])
                        cc += cnt[uu]
                if cc:
                    gy, c = gy + acc, c + cc
            if c or (fault == "inactive_column" and col.size):
                _update(new, "Y", j, gy, hyp, fault)
    tot = _finalize(scal)
    if not frozen & 1:
        _update(new, "mu", (), tot[2], hyp, fault)
    return new, logits, tot[0], tot[1]


def _fresh_state(case):
    t = C.tables_of(case)
    st = {k: dict(w=np.array(t[k], F4)) for k in S.NAMES}
    if case["opt"] == "adam":
        for k in S.NAMES:
            st[k].update(m=np.zeros(np.shape(t[k]), F4), v=np.zeros(np.shape(t[k]), F4))
    return st


def _two_device_steps(case, fault=None):
    st, N = _fresh_state(case), C.implicit()
    powers = (R.B1F, R.B2F)
    bad = []
    for s in range(2):
        u, i, r = C.batch_of(case, s)
        lr, lam = C.hyper_of(case, s)
        new, logits, lossv, regv = _device_step(st, N, (u, i, r), case, s, powers, fault)
        bad += S.check_svdpp_step(st, new, N, u, i, r, opt=case["opt"], loss=case["loss"], item_abs=case["item_abs"],
                                  reg_bias=case["reg_bias"], lam=lam, lr=lr, powers=powers, fresh=s == 0, frozen=case["frozen"],
                                  logits=logits, lossv=lossv, regv=regv)
        st, powers = new, (F4(powers[0] * R.B1F), F4(powers[1] * R.B2F))
    return bad


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_the_device_stand_in_passes_every_check(case):
    bad = _two_device_steps(case)
    assert not bad, bad


def _pick(**kw):
    return [c for c in C.CASES if all(c[k] == v for k, v in kw.items())][0]


ADAM_CASE = _pick(kind="edges", opt="adam", item_abs=True, frozen=0, hyper2=None)
FROZEN_P, FROZEN_Q = _pick(frozen=1 << C.P), _pick(frozen=1 << C.Q)
# fault -> (case, what a violated statement must start with)
FAULTS = {
    "z_last": (ADAM_CASE, "Q"), "neighbour_part": (ADAM_CASE, "Q"), "no_s_in_W": (ADAM_CASE, "Y"), "no_lamcY": (ADAM_CASE, "Y"),
    "c_one": (ADAM_CASE, "Y"), "no_ysq": (ADAM_CASE, "reg"), "items_read_new_P": (ADAM_CASE, "Q"), "sign0_is_1": (ADAM_CASE, "Q"),
    "inactive_column": (ADAM_CASE, "Y."), "v_no_factor:P": (ADAM_CASE, "P: v"), "v_no_factor:Y": (ADAM_CASE, "Y: v"),
    "lr_for_alpha:Y": (ADAM_CASE, "Y: w"), "lr_for_alpha:bu": (ADAM_CASE, "bu: w"), "frozen_m:P": (FROZEN_P, "P.m"),
    "frozen_m:Q": (FROZEN_Q, "Q.m"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_faults_are_rejected(fault):
    """Each fault, planted in the stand-in's two steps, is rejected, and a violated statement names the table:

      z_last            the last entry of a piece dropped from z_u                 Q gradient (and logits, P)
      neighbour_part    another user's piece partial used for z_u                  Q gradient (and logits, P)
      no_s_in_W         s_u missing from W_u                                       Y gradient
      no_lamcY          lam c_u Y[j] missing                                       Y gradient
      c_one             c_u taken as 1                                             Y gradient
      no_ysq            0.5 * ysq missing from the regulariser                     reg
      items_read_new_P  the item side reading the updated P                        Q gradient
      sign0_is_1        sign(0) taken as 1 under item_abs                          Q gradient
      inactive_column   a column of inactive users updated (second step: m decays) Y.m: rows outside the batch changed
      v_no_factor       v built from g g without (1 - b2)                          v does not follow from g
      lr_for_alpha      the apply using lr where alpha belongs                     w does not follow from m and v
      frozen_m          a frozen table's m advanced                                .m: a frozen table changed"""
    case, name = FAULTS[fault]
    assert _two_device_steps(case) == []
    bad = _two_device_steps(case, fault)
    print("fault %s: %d statements violated, first: %s" % (fault, len(bad), bad[:1]))
    assert any(b.startswith(name) for b in bad), "fault %s passes, or no statement names %s: %s" % (fault, name, bad)


def test_cases_cover_what_the_kernels_are_built_around():
    from tests import widths as W
    edges = [c for c in C.CASES if c["kind"] == "edges"]
    assert {c["D"] for c in edges} >= set(W.SVDPP) | {1, 5, 16}
    assert {c["tail"] for c in edges} >= {65, 129}
    assert {c["frozen"] for c in C.CASES if c["opt"] == "adam"} >= {1 << b for b in range(6)} | {(1 << C.P) | (1 << C.Q)}
    assert {c["kind"] for c in C.CASES} == {"edges", "one", "oneuser"}
    assert any(c["hyper2"] for c in C.CASES)
    assert any(c["item_abs"] and c["kind"] == "edges" for c in C.CASES)
    for key in ("loss", "item_abs", "reg_bias", "opt"):
        assert len({c[key] for c in edges}) == 2, key
