"""One BPR training step stated per row (include/tfrecomm.h "BPR"): the float64 gradient sum of the contract
in tests/bpr_ref.py for P, Q and bi, a first-order bound on what float32 may lose of it, a float32 restatement in contract
order that sets the limit, and the consistency checks of tests/step_ref.py on the device's own moments and weights.  mu
and bu are never read or written: every slot of theirs is held to identical bits.  NumPy only.

A triple (u, i, j) with j = -1 is skipped: it contributes nothing and touches nothing.  Per live triple
    x = (P[u] . Q'[i] + bi[i]) - (P[u] . Q'[j] + bi[j]),  g = -sigmoid(-x)
    dP[u] += g (Q'[i] - Q'[j]) + lam P[u];  dQ[i] += g P[u] sign_i + lam Q[i];  dQ[j] += -g P[u] sign_j + lam Q[j];  dbi[i] += g;  dbi[j] -= g
"""
import numpy as np

from oracle import svd_oracle as so
from tests import bpr_ref as BR
from tests import step_ref as R
from tests.fm_ref import _held

NAMES = ("P", "Q", "bi")
HELD = ("mu", "bu")
TID = {"mu": BR.MU, "bu": BR.BU, "bi": BR.BI, "P": BR.PF, "Q": BR.QF}


def _softplus_neg(x):
    return np.maximum(-x, 0) + np.log1p(np.exp(-np.abs(x)))


def bpr_step_grads(t, u, i, j, item_abs, reg_bias, lam):
    """({name: (G, E, n)}, terms) for P, Q, bi over the live triples: G the float64 gradient sum of the contract (dense, zero
    on untouched rows), E the first-order float32 loss bound in units of eps32, n the entries per row - an item's n counts
    its occurrences in both roles.  ``terms``: x, X, g per live triple, the data loss and the regulariser with their bounds.

    x:    the prediction error is that of x = (di + bi) - (dj + bj): the terms p_d q~_d of both dots and the two biases by
          their magnitudes, X = sum_d |p| (|q~_i| + |q~_j|) + |bi_i| + |bi_j|.
    g:    g = -1 / (1 + exp(x)), |dg/dx| <= 1/4.  expf is off by up to an ulp (2 eps32), which moves g by
          |g| (1 - |g|) x 2; the addition and the division round once each: delta = X / 4 + 4 |g|.
    dP:   delta |q~_i - q~_j| (the error of g), |g| |q~_i - q~_j| (the subtraction), lam |p|, 2 |occurrence| (the fused
          sum of the two, and one rounding as a term of the row's sum).
    dQ:   per occurrence delta |p|, |g p| and lam |q| (the two products), 2 |occurrence|; where sign(Q) = 0 the first two
          vanish exactly.
    dbi:  delta, lam |bi| under reg_bias, 2 |occurrence|.
    loss: sum_b (|g_b| X_b + 2 |l_b|) as tests/fm_ref.py.   regulariser: 3 x the triple's term (tests/svdpp_step_ref.py)."""
    P, Q, bi = (np.asarray(t[k], np.float64) for k in ("P", "Q", "bi"))
    keep = np.asarray(j) >= 0
    u, i, j = (np.asarray(a, np.int64)[keep] for a in (u, i, j))
    U, I = P.shape[0], Q.shape[0]
    Qt = np.abs(Q) if item_abs else Q
    sg = np.sign(Q) if item_abs else np.ones_like(Q)
    p = P[u]
    x = (np.sum(p * Qt[i], 1) + bi[i]) - (np.sum(p * Qt[j], 1) + bi[j])
    X = np.sum(np.abs(p) * (np.abs(Qt[i]) + np.abs(Qt[j])), 1) + np.abs(bi[i]) + np.abs(bi[j])
    g = -1.0 / (1.0 + np.exp(x))
    delta = X / 4 + 4 * np.abs(g)
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
    lrow = _softplus_neg(x)
    rk = 0.5 * (np.sum(p * p, 1) + np.sum(Q[i] ** 2, 1) + np.sum(Q[j] ** 2, 1))
    if reg_bias:
        rk = rk + 0.5 * (bi[i] ** 2 + bi[j] ** 2)
    B = np.int64(u.size)
    terms = dict(x=x, X=X, g=g, loss=(np.float64(lrow.sum()), np.float64(np.sum(np.abs(g) * X + 2 * np.abs(lrow))), B),
                 reg=(np.float64(rk.sum()), np.float64(3 * rk.sum()), B))
    return out, terms


def f32_bpr(t, u, i, j, item_abs, reg_bias, lam):
    """The same numbers in float32 arithmetic in the contract's order, the way ``bpr_ref.gradients`` forms them on float32
    tables: ``np.add.at`` in batch order, an item's positive occurrences before its negative ones.  dict of the three
    gradients, loss and reg.  It supplies c_ref."""
    f4 = np.float32
    t4 = {TID[k]: np.asarray(t[k], f4) for k in ("P", "Q", "bi")}
    G = BR.gradients(t4, u, i, j, f4(lam), item_abs, reg_bias)
    out = {"P": G[BR.PF][0], "Q": G[BR.QF][0], "bi": G[BR.BI][0]}
    keep = np.asarray(j) >= 0
    u, i, j = (np.asarray(a, np.int64)[keep] for a in (u, i, j))
    P, Q, bi = t4[BR.PF], t4[BR.QF], t4[BR.BI]
    Qt = np.abs(Q) if item_abs else Q
    x = (np.sum(P[u] * Qt[i], 1, dtype=f4) + bi[i]) - (np.sum(P[u] * Qt[j], 1, dtype=f4) + bi[j])
    lrow = _softplus_neg(x).astype(f4)
    rk = f4(0.5) * (np.sum(P[u] ** 2, 1, dtype=f4) + np.sum(Q[i] ** 2, 1, dtype=f4) + np.sum(Q[j] ** 2, 1, dtype=f4))
    if reg_bias:
        rk = rk + f4(0.5) * (bi[i] ** 2 + bi[j] ** 2)
    out["loss"] = np.cumsum(lrow, dtype=f4)[-1] if u.size else f4(0)
    out["reg"] = np.cumsum(rk, dtype=f4)[-1] if u.size else f4(0)
    assert all(np.asarray(v).dtype == f4 for v in out.values()), {k: np.asarray(v).dtype for k, v in out.items()}
    return out


def check_bpr_step(before, after, u, i, j, *, opt, item_abs, reg_bias, lam, lr, powers, fresh, frozen=0, lossv=None, regv=None,
                   report=None):
    """Every per-row statement about one BPR step.  ``before`` / ``after``: {name: dict(w=, m=, v=)} of float32 arrays read
    around the step for mu, bu, bi, P, Q (m, v absent under SGD); ``j`` the negatives the step used (-1 = skipped).  Per
    table and run-length class: the gradient the device used lies within ``limit_from(c_ref)`` x eps32 x E of the float64
    sum over the live triples; v follows from g and the previous v; w from the device's own m and v; every slot of a row
    no live triple names and of a frozen table keeps its bits (``step_ref.check_table``); every slot of mu and bu keeps
    its bits.  ``lossv`` and ``regv`` are held as sums of one row.  Returns the violated statements."""
    tabs = {k: before[k]["w"] for k in NAMES}
    ref, t = bpr_step_grads(tabs, u, i, j, item_abs, reg_bias, lam)
    f32 = f32_bpr(tabs, u, i, j, item_abs, reg_bias, lam)
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
                bad.append("%s.%s: a BPR step changed a table it never reads or writes" % (name, slot))
    for what, got in (("loss", lossv), ("reg", regv)):
        if got is not None:
            G, E, n = (np.reshape(a, (1,)) for a in t[what])
            bad += _held(what, np.reshape(np.float64(got), (1,)), G, E, n, R.ratio(np.reshape(f32[what], (1,)), G, E, n), report)
    return bad
