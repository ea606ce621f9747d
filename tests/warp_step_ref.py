"""One WARP training step stated per row (include/tfrecomm.h "WARP"), in the manner of
tests/bpr_step_ref.py: the float64 gradient sum of the contract in tests/warp_ref.py for P, Q and bi given the negatives and
trial counts the step used, a first-order bound on what float32 may lose of it, a float32 restatement in contract order that
sets the limit, and the consistency checks of tests/step_ref.py on the device's own moments and weights.  mu and bu are
never read or written: every slot of theirs is held to identical bits.  NumPy only.

A triple (u, i, j) with j = -1 is skipped: it contributes nothing and touches nothing.  Per live triple, N its trial count,
    x = (P[u] . Q'[i] + bi[i]) - (P[u] . Q'[j] + bi[j]),  w = log(max(1, (I - 1) // N)),  g = -w if x < margin else 0
    dP[u] += g (Q'[i] - Q'[j]) + lam P[u];  dQ[i] += g P[u] sign_i + lam Q[i];  dQ[j] += -g P[u] sign_j + lam Q[j];  dbi[i] += g;  dbi[j] -= g
"""
import numpy as np

from oracle import svd_oracle as so
from tests import bpr_step_ref as BS
from tests import step_ref as R
from tests import warp_ref as WR
from tests.fm_ref import _held

NAMES, HELD, TID = BS.NAMES, BS.HELD, BS.TID


def warp_step_grads(t, u, i, j, trials, margin, item_abs, reg_bias, lam):
    """({name: (G, E, n)}, terms) for P, Q, bi over the live triples, as ``bpr_step_ref.bpr_step_grads`` gives them.

    g:    g = -w or 0: no expf in it.  w = logf(integer) is off by up to 2 ulp (4 eps32): delta = 4 |w|.  The hinge decides
          on x: the float32 x is within tol = BAND eps32 (X + |margin|) of the float64 one (``warp_ref.examine``), so the
          decision can differ only where |margin - x| <= tol; there g may be either value, and delta gains w / eps32 (the
          whole of w).  A searched triple is live because the device found x < margin on the very bits the step uses, so
          there too only an in-band x can disagree.
    dP, dQ, dbi: ``bpr_step_grads``' terms with this delta.
    loss: sum_b (w_b X_b + 6 |l_b|) (the error of x, of w, the subtraction and the product), plus w tol / eps32 in the band.
    regulariser: 3 x the triple's term."""
    P, Q, bi = (np.asarray(t[k], np.float64) for k in ("P", "Q", "bi"))
    keep = np.asarray(j) >= 0
    u, i, j, N = (np.asarray(a, np.int64)[keep] for a in (u, i, j, trials))
    U, I = P.shape[0], Q.shape[0]
    w = WR.weights(I, N)
    Qt = np.abs(Q) if item_abs else Q
    sg = np.sign(Q) if item_abs else np.ones_like(Q)
    p = P[u]
    x = (np.sum(p * Qt[i], 1) + bi[i]) - (np.sum(p * Qt[j], 1) + bi[j])
    X = np.sum(np.abs(p) * (np.abs(Qt[i]) + np.abs(Qt[j])), 1) + np.abs(bi[i]) + np.abs(bi[j])
    tol = WR.BAND * WR.EPS32 * (X + abs(margin))
    band = np.abs(margin - x) <= tol
    g = np.where(x < margin, -w, 0.0)
    delta = 4 * w + np.where(band, w / WR.EPS32, 0.0)
    dq = Qt[i] - Qt[j]
    oP = g[:, None] * dq + lam * p
    EP = (delta + np.abs(g))[:, None] * np.abs(dq) + lam * np.abs(p) + 2 * np.abs(oP)
    ids = np.concatenate((i, j))
    gg = np.concatenate((g, -g))
    pp, dd = np.concatenate((p, p)), np.concatenate((delta, delta))
    oQ = gg[:, None] * pp * sg[ids] + lam * Q[ids]
    EQ = np.abs(sg[ids]) * (dd[:, None] * np.abs(pp) + np.abs(gg[:, None] * pp)) + lam * np.abs(Q[ids]) + 2 * np.abs(oQ)
    ob, Eb = gg.copy(), dd.copy()
    if reg_bias:
        ob, Eb = ob + lam * bi[ids], Eb + lam * np.abs(bi[ids])
    Eb = Eb + 2 * np.abs(ob)
    nu = np.bincount(u, minlength=U).astype(np.int64)
    ni = np.bincount(ids, minlength=I).astype(np.int64)
    out = {
        "P": (R.seg_sum(oP, u, U), R.seg_sum(EP, u, U), nu[:, None]),
        "Q": (R.seg_sum(oQ, ids, I), R.seg_sum(EQ, ids, I), ni[:, None]),
        "bi": (R.seg_sum(ob, ids, I), R.seg_sum(Eb, ids, I), ni),
    }
    lrow = w * np.maximum(0.0, margin - x)
    rk = 0.5 * (np.sum(p * p, 1) + np.sum(Q[i] ** 2, 1) + np.sum(Q[j] ** 2, 1))
    if reg_bias:
        rk = rk + 0.5 * (bi[i] ** 2 + bi[j] ** 2)
    B = np.int64(u.size)
    El = np.sum(w * X + 6 * np.abs(lrow) + np.where(band, w * tol / WR.EPS32, 0.0))
    terms = dict(x=x, X=X, g=g, w=w, band=band, loss=(np.float64(lrow.sum()), np.float64(El), B),
                 reg=(np.float64(rk.sum()), np.float64(3 * rk.sum()), B))
    return out, terms


def f32_warp(t, u, i, j, trials, margin, item_abs, reg_bias, lam):
    """The same numbers in float32 arithmetic in the contract's order, the way ``warp_ref.gradients`` forms them on float32
    tables: ``np.add.at`` in batch order, an item's positive occurrences before its negative ones.  It supplies c_ref."""
    f4 = np.float32
    t4 = {TID[k]: np.asarray(t[k], f4) for k in ("P", "Q", "bi")}
    I = t4[WR.QF].shape[0]
    w = WR.weights(I, np.where(np.asarray(j) >= 0, trials, 0)).astype(f4)
    G = WR.gradients(t4, u, i, j, w, f4(margin), f4(lam), item_abs, reg_bias)
    out = {"P": G[WR.PF][0], "Q": G[WR.QF][0], "bi": G[WR.BI][0]}
    keep = np.asarray(j) >= 0
    u, i, j = (np.asarray(a, np.int64)[keep] for a in (u, i, j))
    w = w[keep]
    P, Q, bi = t4[WR.PF], t4[WR.QF], t4[WR.BI]
    Qt = np.abs(Q) if item_abs else Q
    x = (np.sum(P[u] * Qt[i], 1, dtype=f4) + bi[i]) - (np.sum(P[u] * Qt[j], 1, dtype=f4) + bi[j])
    lrow = (w * np.maximum(f4(0), f4(margin) - x)).astype(f4)
    rk = f4(0.5) * (np.sum(P[u] ** 2, 1, dtype=f4) + np.sum(Q[i] ** 2, 1, dtype=f4) + np.sum(Q[j] ** 2, 1, dtype=f4))
    if reg_bias:
        rk = rk + f4(0.5) * (bi[i] ** 2 + bi[j] ** 2)
    out["loss"] = np.cumsum(lrow, dtype=f4)[-1] if u.size else f4(0)
    out["reg"] = np.cumsum(rk, dtype=f4)[-1] if u.size else f4(0)
    assert all(np.asarray(v).dtype == f4 for v in out.values()), {k: np.asarray(v).dtype for k, v in out.items()}
    return out


def check_warp_step(before, after, u, i, j, trials, *, margin, opt, item_abs, reg_bias, lam, lr, powers, fresh, frozen=0,
                    lossv=None, regv=None, report=None):
    """Every per-row statement about one WARP step, as ``bpr_step_ref.check_bpr_step`` makes them for a BPR step: ``j`` and
    ``trials`` are the negatives (-1 = skipped) and trial counts the step used.  Returns the violated statements."""
    tabs = {k: before[k]["w"] for k in NAMES}
    ref, t = warp_step_grads(tabs, u, i, j, trials, margin, item_abs, reg_bias, lam)
    f32 = f32_warp(tabs, u, i, j, trials, margin, item_abs, reg_bias, lam)
    adam = opt == so.ADAM
    alpha = R.alpha_f32(lr, *powers) if adam else 0.0
    bad = []
    for name in NAMES:
        G, E, n = ref[name]
        R.check_table(bad, name, G, E, n, before[name], after[name], f32[name], adam=adam, tf1=False, fresh=fresh, lr=lr,
                      alpha=alpha, frozen=frozen >> TID[name] & 1, report=report)
    for name in HELD:
        for slot in before[name]:
            if not R.same_bits(before[name][slot], after[name][slot]):
                bad.append("%s.%s: a WARP step changed a table it never reads or writes" % (name, slot))
    for what, got in (("loss", lossv), ("reg", regv)):
        if got is not None:
            G, E, n = (np.reshape(a, (1,)) for a in t[what])
            bad += _held(what, np.reshape(np.float64(got), (1,)), G, E, n, R.ratio(np.reshape(f32[what], (1,)), G, E, n), report)
    return bad
