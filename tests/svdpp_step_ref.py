"""One SVD++ training step stated per row (include/tfrecomm.h tfr_svdpp_*): the float64 gradient sum of the
contract in tests/svdpp_ref.py for P, Q, bu, bi, mu and Y, a first-order bound on what float32 may lose of it, a float32
restatement in contract order that sets the limit, and the consistency checks of tests/step_ref.py on the device's own
moments and weights.  NumPy only.

    s_u = |N(u)|^-1/2,  z_u = s_u sum_{j in N(u)} Y[j],  e_k = P[u_k] + z_{u_k},  x_k = ((e_k . Q'[i_k] + mu) + bu) + bi
    dP = g Q' + lam P    dQ = g e sign + lam Q    W_u = s_u sum_{k in u} g_k Q'[i_k]    GY[j] = sum_{u active, j in N(u)} (W_u + lam c_u Y[j])
"""
import numpy as np

from oracle import svd_oracle as so
from tests import step_ref as R
from tests import svdpp_ref as PR
from tests.fm_ref import _held, _row_loss

NAMES = ("P", "Q", "bu", "bi", "mu", "Y")
TID = {"mu": PR.MU, "bu": PR.BU, "bi": PR.BI, "P": PR.PF, "Q": PR.QF, "Y": PR.YF}


def by_id(t, dtype):
    """the tables keyed as tests/svdpp_ref.py wants them"""
    return {TID[k]: np.asarray(t[k], dtype) for k in NAMES}


def svdpp_step_grads(t, indptr, items, u, i, r, loss, item_abs, reg_bias, lam):
    """({name: (G, E, n)}, terms) for P, Q, bu, bi, mu, Y: G the float64 gradient sum of the contract (dense, zero on
    untouched rows), E the first-order float32 loss bound in units of eps32, n the entries per row - for Y the number of
    active users in column j, the length of the sum the Y kernels form.  ``terms``: x, X, g, the data loss and the
    regulariser with their bounds, |N(u)| per entry.

    z_u:  the sum over N(u) is a float32 sum, off by eps32 A_u per element, A_u = sum_j |Y[j]| (its growth with |N(u)|
          is what the float32 restatement measures); s_u = 1 / sqrtf(.) rounds twice and s_u * sum once: the error of
          z_u is Ze_u = s_u A_u + 3 |z_u|.
    e_k:  the addition P + z rounds: Ze_u + |e_k|.
    x_k:  the error of e reaches the dot through |Q'|; the products and their sum lose one rounding of |e Q'| more; mu and
          the biases by their magnitudes: X_k = sum_d ((Ze + |e|) |Q'| + |e Q'|) + |mu| + |bu| + |bi|.
    g_k:  delta_k = X_k + |r_k| under mse (the subtraction), X_k / 4 + |g_k| under nll (tests/step_ref.py).
    dP:   delta |Q'| (the error of g), |g Q'| and lam |P| (the two products), 2 |occurrence| (their sum, and one rounding
          as a term of the row's sum).
    dQ:   delta |e|, |g| (Ze + |e|) (the stored e_k carries its own error), |g e| and lam |Q|, 2 |occurrence|; where
          sign(Q) = 0 the first three vanish exactly.
    bu, bi: delta, lam |b| under reg_bias, 2 |occurrence|.   mu: delta + |g| per entry.
    W_u:  s_u sum_k (delta_k |Q'| + 2 |g_k Q'|) (the error of each g_k, the product and the running sum) + 3 |W_u| (s_u and
          the product): EW_u.  It reaches every Y row of N(u).
    GY:   per active user of the column, the term T = W_u + lam c_u Y[j]: EW_u + 2 lam c_u |Y[j]| (lam * c_u and its
          product with Y[j]) + 2 |T| (the sum, and one rounding as a term of the column's sum).
    loss: sum_k (|g_k| X_k + 2 |l_k|) as tests/fm_ref.py.   regulariser: each entry's 1/2 (|P|^2 + |Q|^2 + sum_N |Y|^2
          (+ bu^2 + bi^2)) is a sum of squares formed in float32 (one rounding of its size), rounded where it is formed
          and where it is added: 3 x the entry's term."""
    t = {k: np.asarray(t[k], np.float64) for k in NAMES}
    P, Q, bu, bi, mu, Y = (t[k] for k in ("P", "Q", "bu", "bi", "mu", "Y"))
    indptr, items = np.asarray(indptr, np.int64), np.asarray(items, np.int64)
    u, i, r = np.asarray(u, np.int64), np.asarray(i, np.int64), np.asarray(r, np.float64)
    U, I, D = P.shape[0], Q.shape[0], P.shape[1]
    users = np.unique(u)
    pos = np.searchsorted(users, u)
    nN = (indptr[users + 1] - indptr[users]).astype(np.int64)
    s = np.where(nN > 0, 1.0 / np.sqrt(np.maximum(nN, 1)), 0.0)
    sumY, A, ysq = np.zeros((users.size, D)), np.zeros((users.size, D)), np.zeros(users.size)
    for x, uu in enumerate(users):
        rows = Y[items[indptr[uu]:indptr[uu + 1]]]
        sumY[x], A[x], ysq[x] = rows.sum(axis=0), np.abs(rows).sum(axis=0), np.sum(rows * rows)
    z = s[:, None] * sumY
    Ze = s[:, None] * A + 3 * np.abs(z)
    e = (P[users] + z)[pos]
    Zk = Ze[pos]
    pu, qi = P[u], Q[i]
    qt = np.abs(qi) if item_abs else qi
    sg = np.sign(qi) if item_abs else np.ones_like(qi)
    aq = np.abs(qt)
    x = ((np.sum(e * qt, axis=1) + mu) + bu[u]) + bi[i]
    X = np.sum((Zk + np.abs(e)) * aq + np.abs(e * qt), axis=1) + abs(float(mu)) + np.abs(bu[u]) + np.abs(bi[i])
    g = so.dlogits(x, r, loss)
    delta = X + np.abs(r) if loss == so.MSE else X / 4 + np.abs(g)
    ag = np.abs(g)[:, None]
    oP = g[:, None] * qt + lam * pu
    EP = delta[:, None] * aq + ag * aq + lam * np.abs(pu) + 2 * np.abs(oP)
    oQ = g[:, None] * e * sg + lam * qi
    EQ = np.abs(sg) * (delta[:, None] * np.abs(e) + ag * (Zk + np.abs(e)) + ag * np.abs(e)) + lam * np.abs(qi) + 2 * np.abs(oQ)
    obu, obi = g.copy(), g.copy()
    Ebu, Ebi = delta.copy(), delta.copy()
    if reg_bias:
        obu, obi = obu + lam * bu[u], obi + lam * bi[i]
        Ebu, Ebi = Ebu + lam * np.abs(bu[u]), Ebi + lam * np.abs(bi[i])
    Ebu, Ebi = Ebu + 2 * np.abs(obu), Ebi + 2 * np.abs(obi)
    W = s[:, None] * R.seg_sum(g[:, None] * qt, pos, users.size)
    EW = s[:, None] * R.seg_sum(delta[:, None] * aq + 2 * ag * aq, pos, users.size) + 3 * np.abs(W)
    c = np.bincount(pos, minlength=users.size).astype(np.int64)
    GY, EY, nY = np.zeros_like(Y), np.zeros_like(Y), np.zeros(I, np.int64)
    for k, uu in enumerate(users):
        js = items[indptr[uu]:indptr[uu + 1]]
        T = W[k] + lam * c[k] * Y[js]
        GY[js] += T
        EY[js] += EW[k] + 2 * lam * c[k] * np.abs(Y[js]) + 2 * np.abs(T)
        nY[js] += 1
    nu = np.bincount(u, minlength=U).astype(np.int64)
    ni = np.bincount(i, minlength=I).astype(np.int64)
    out = {
        "P": (R.seg_sum(oP, u, U), R.seg_sum(EP, u, U), nu[:, None]),
        "Q": (R.seg_sum(oQ, i, I), R.seg_sum(EQ, i, I), ni[:, None]),
        "bu": (R.seg_sum(obu, u, U), R.seg_sum(Ebu, u, U), nu),
        "bi": (R.seg_sum(obi, i, I), R.seg_sum(Ebi, i, I), ni),
        "mu": (np.float64(g.sum()), np.float64(np.sum(np.abs(g) + delta)), np.int64(u.size)),
        "Y": (GY, EY, nY[:, None]),
    }
    lrow = _row_loss(x, r, loss)
    rk = 0.5 * (np.sum(pu * pu, axis=1) + np.sum(qi * qi, axis=1) + ysq[pos])
    if reg_bias:
        rk = rk + 0.5 * (bu[u] ** 2 + bi[i] ** 2)
    B = np.int64(u.size)
    terms = dict(x=x, X=X, g=g, nN=nN[pos], W=W, c=c, users=users,
                 loss=(np.float64(lrow.sum()), np.float64(np.sum(np.abs(g) * X + 2 * np.abs(lrow))), B),
                 reg=(np.float64(rk.sum()), np.float64(3 * rk.sum()), B))
    return out, terms


def f32_svdpp(t, indptr, items, u, i, r, loss, item_abs, reg_bias, lam):
    """The same numbers in float32 arithmetic in the contract's order, the way ``svdpp_ref.SvdppRef(dtype=np.float32)`` forms
    them: z_u a sum over N(u) in row order, every occurrence sum by ``np.add.at`` in batch order, GY over the active users
    ascending.  dict of the six gradients, x, loss and reg.  It supplies c_ref."""
    f4 = np.float32
    t = by_id(t, f4)
    indptr, items = np.asarray(indptr, np.int64), np.asarray(items, np.int64)
    u, i, r = np.asarray(u, np.int64), np.asarray(i, np.int64), np.asarray(r, f4)
    U, I = t[PR.PF].shape[0], t[PR.QF].shape[0]
    x = PR.forward(t, indptr, items, u, i, item_abs).astype(f4)
    g = so.dlogits(x, r, loss).astype(f4)
    occ = PR.occurrences(t, indptr, items, u, i, g, item_abs, reg_bias, lam)
    out = dict(x=x)
    out["P"], out["Q"] = so.segment_sum(occ["P"].astype(f4), u, U), so.segment_sum(occ["Q"].astype(f4), i, I)
    out["bu"], out["bi"] = so.segment_sum(occ["bu"].astype(f4), u, U), so.segment_sum(occ["bi"].astype(f4), i, I)
    out["mu"] = np.cumsum(g, dtype=f4)[-1] if g.size else f4(0)
    out["Y"] = PR.y_gradient(t, indptr, items, u, occ["W"].astype(f4), occ["c"], occ["users"], lam)[0]
    lrow = _row_loss(x, r, loss).astype(f4)
    out["loss"] = np.cumsum(lrow, dtype=f4)[-1] if g.size else f4(0)
    _, _, ysq = PR.implicit_parts(t[PR.YF], indptr, items, u)
    P, Q, bu, bi = t[PR.PF], t[PR.QF], t[PR.BU], t[PR.BI]
    rk = f4(0.5) * (np.sum(P[u] * P[u], axis=1, dtype=f4) + np.sum(Q[i] * Q[i], axis=1, dtype=f4) + ysq)
    if reg_bias:
        rk = rk + f4(0.5) * (bu[u] * bu[u] + bi[i] * bi[i])
    out["reg"] = np.cumsum(rk, dtype=f4)[-1] if g.size else f4(0)
    assert all(np.asarray(v).dtype == f4 for v in out.values()), {k: np.asarray(v).dtype for k, v in out.items()}
    return out


def touched_y(indptr, items, u, I):
    """bool [I]: some active user has j in N(u)"""
    out = np.zeros(I, bool)
    for uu in np.unique(np.asarray(u, np.int64)):
        out[items[indptr[uu]:indptr[uu + 1]]] = True
    return out


def check_svdpp_step(before, after, N, u, i, r, *, opt, loss, item_abs, reg_bias, lam, lr, powers, fresh, frozen=0,
                     logits=None, lossv=None, regv=None, report=None):
    """Every per-row statement about one SVD++ step.  ``before`` / ``after``: {name: dict(w=, m=, v=)} of float32 arrays
    read around the step for the six tables (m, v absent under SGD); ``N`` = (indptr, items); ``powers`` = (b1p, b2p)
    before the step; ``fresh``: the slots were all zero before; ``frozen``: the mask of bits 0..5.  Per table (mu as a
    table of one row) and run-length class: the gradient the device used lies within ``limit_from(c_ref)`` x eps32 x E of
    the float64 sum; v follows from g and the previous v; w from the device's own m and v; every slot of a row outside the
    batch - for Y: of a column without an active user - and of a frozen table keeps its bits (``step_ref.check_table``).
    ``logits`` are held per entry, ``lossv`` and ``regv`` as sums of one row.  Returns the violated statements."""
    indptr, items = N
    tabs = {k: before[k]["w"] for k in NAMES}
    ref, t = svdpp_step_grads(tabs, indptr, items, u, i, r, loss, item_abs, reg_bias, lam)
    f32 = f32_svdpp(tabs, indptr, items, u, i, r, loss, item_abs, reg_bias, lam)
    adam = opt == so.ADAM
    alpha = R.alpha_f32(lr, *powers) if adam else 0.0
    bad = []
    for name in NAMES:
        G, E, n = ref[name]
        R.check_table(bad, name, G, E, n, before[name], after[name], f32[name], adam=adam, tf1=False, fresh=fresh, lr=lr,
                      alpha=alpha, frozen=frozen >> TID[name] & 1, report=report)
    if logits is not None:
        bad += _held("logits", np.asarray(logits, np.float64), t["x"], t["X"], t["nN"], R.ratio(f32["x"], t["x"], t["X"], t["nN"]),
                     report)
    for what, got in (("loss", lossv), ("reg", regv)):
        if got is not None:
            G, E, n = (np.reshape(a, (1,)) for a in t[what])
            bad += _held(what, np.reshape(np.float64(got), (1,)), G, E, n, R.ratio(np.reshape(f32[what], (1,)), G, E, n), report)
    return bad
