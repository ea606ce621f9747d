"""Float64 restatement of the SVD++ step (include/tfrecomm.h tfr_svdpp_*) - the truth the device is checked
against.  Built on the SVD oracle's pieces, so that with Y = 0 (and Y frozen) every table takes exactly the SVD step.

    s_u   = 1/sqrt(|N(u)|) (0 for an empty row),  z_u = s_u * sum_{j in N(u)} Y[j],  e_k = P[u_k] + z_{u_k}
    logit = ((dot(e_k, Q'[i_k]) + mu) + bu[u_k]) + bi[i_k]                          Q' = |Q| under item_abs
    cost  = data_loss + lam * (svd regulariser + sum_k 1/2 sum_{j in N(u_k)} ||Y[j]||^2)
    per occurrence, g_k = d loss / d logit_k:
      dP = g Q'[i] + lam P[u];  dQ = g e_k (* sign(Q[i]) under item_abs) + lam Q[i];  biases and mu as in SVD
      dY[j] += g_k s_u Q'[i_k] + lam Y[j]   for every j in N(u_k)
      = per active user u: W_u = s_u sum_{k in u} g_k Q'[i_k], c_u = #entries of u;  GY[j] = sum_{u active, j in N(u)} (W_u + lam c_u Y[j])
"""
from __future__ import annotations

import numpy as np

from oracle import svd_oracle as so

MU, BU, BI, PF, QF, YF = 0, 1, 2, 3, 4, 5


def implicit_parts(Y, indptr, items, users):
    """(z [n, D], s [n], ysq [n]) for each of ``users``: z_u, s_u and sum_{j in N(u)} ||Y[j]||^2."""
    dt = Y.dtype
    n = len(users)
    z = np.zeros((n, Y.shape[1]), dt)
    s = np.zeros(n, dt)
    ysq = np.zeros(n, dt)
    for k, u in enumerate(users):
        lo, hi = int(indptr[u]), int(indptr[u + 1])
        if hi > lo:
            rows = Y[items[lo:hi]]
            s[k] = dt.type(1) / np.sqrt(dt.type(hi - lo))
            z[k] = s[k] * rows.sum(axis=0)
            ysq[k] = np.sum(rows * rows)
    return z, s, ysq


def forward(t, indptr, items, u, i, item_abs=False):
    mu, bu, bi, P, Q, Y = (t[x] for x in (MU, BU, BI, PF, QF, YF))
    z, _, _ = implicit_parts(Y, indptr, items, u)
    e = P[u] + z
    qi = Q[i]
    qt = np.abs(qi) if item_abs else qi
    logits = np.sum(e * qt, axis=1)
    return ((logits + mu) + bu[u]) + bi[i]


def regularizer(t, indptr, items, u, i, reg_bias=False):
    dt = t[PF].dtype
    _, _, ysq = implicit_parts(t[YF], indptr, items, u)
    return dt.type(so.regularizer(t[PF], t[QF], t[BU], t[BI], u, i, reg_bias) + dt.type(0.5) * np.sum(ysq))


def cost(t, indptr, items, u, i, r, loss="mse", item_abs=False, reg_bias=False, lam=0.05):
    x = forward(t, indptr, items, u, i, item_abs)
    return so.data_loss(x, r, loss) + lam * regularizer(t, indptr, items, u, i, reg_bias)


def gradients(t, indptr, items, u, i, r, loss="mse", item_abs=False, reg_bias=False, lam=0.05):
    """Dense d cost / d table for every table: the occurrence sums of the contract (for finite differences and for the
    SGD lr = 1 recovery of the device's gradients)."""
    dt = t[PF].dtype
    mu, bu, bi, P, Q, Y = (t[x] for x in (MU, BU, BI, PF, QF, YF))
    x = forward(t, indptr, items, u, i, item_abs)
    g = so.dlogits(x, r, loss)
    occ = occurrences(t, indptr, items, u, i, g, item_abs, reg_bias, lam)
    G = {MU: np.array(occ["mu"], dt), BU: np.zeros_like(bu), BI: np.zeros_like(bi), PF: np.zeros_like(P),
         QF: np.zeros_like(Q)}
    np.add.at(G[BU], u, occ["bu"])
    np.add.at(G[BI], i, occ["bi"])
    np.add.at(G[PF], u, occ["P"])
    np.add.at(G[QF], i, occ["Q"])
    G[YF] = y_gradient(t, indptr, items, u, occ["W"], occ["c"], occ["users"], lam)[0]
    return G


def occurrences(t, indptr, items, u, i, g, item_abs, reg_bias, lam):
    """Per-entry gradient rows of the five SVD tables, and the per-active-user W_u, c_u of the Y gradient."""
    dt = t[PF].dtype
    lam = dt.type(lam)
    bu, bi, P, Q, Y = (t[x] for x in (BU, BI, PF, QF, YF))
    z, s, _ = implicit_parts(Y, indptr, items, u)
    pu, qi = P[u], Q[i]
    e = pu + z
    qt = np.abs(qi) if item_abs else qi
    dP = g[:, None] * qt + lam * pu
    dQ = (g[:, None] * e * np.sign(qi) if item_abs else g[:, None] * e) + lam * qi
    dbu, dbi = g.copy(), g.copy()
    if reg_bias:
        dbu = dbu + lam * bu[u]
        dbi = dbi + lam * bi[i]
    users = np.unique(u)
    W = np.zeros((users.size, P.shape[1]), dt)
    c = np.zeros(users.size, np.int64)
    pos = np.searchsorted(users, u)
    np.add.at(W, pos, g[:, None] * qt)
    np.add.at(c, pos, 1)
    _, su, _ = implicit_parts(Y, indptr, items, users)
    W = su[:, None] * W
    return dict(P=dP, Q=dQ, bu=dbu, bi=dbi, mu=dt.type(np.sum(g)), W=W, c=c, users=users)


def y_gradient(t, indptr, items, u, W, c, users, lam):
    """(GY dense [I, D], touched rows): GY[j] = sum over active users u with j in N(u) of W_u + lam c_u Y[j]."""
    Y = t[YF]
    dt = Y.dtype
    GY = np.zeros_like(Y)
    touched = np.zeros(Y.shape[0], bool)
    for x, uu in enumerate(users):
        js = items[int(indptr[uu]):int(indptr[uu + 1])]
        GY[js] += W[x] + dt.type(lam) * dt.type(c[x]) * Y[js]
        touched[js] = True
    return GY, np.flatnonzero(touched)


class SvdppRef:
    """Whole-model restatement: the six tables (+ lazy-Adam slots), SGD or lazy Adam, frozen bits 0..5."""

    def __init__(self, U, I, D, indptr, items, *, loss="mse", item_abs=False, reg_bias=False, optimizer="adam",
                 lr=1e-3, reg=0.05, dtype=np.float64):
        self.U, self.I, self.D = int(U), int(I), int(D)
        self.indptr = np.asarray(indptr, np.int64)
        self.items = np.asarray(items, np.int64)
        self.loss, self.item_abs, self.reg_bias, self.optimizer = loss, bool(item_abs), bool(reg_bias), optimizer
        self.lr, self.reg = lr, reg
        self.dt = np.dtype(dtype)
        dt = self.dt
        self.t = {MU: np.zeros((), dt), BU: np.zeros(self.U, dt), BI: np.zeros(self.I, dt),
                  PF: np.zeros((self.U, self.D), dt), QF: np.zeros((self.I, self.D), dt), YF: np.zeros((self.I, self.D), dt)}
        self.slots = {k: so.AdamState(v.shape, dt) for k, v in self.t.items()}
        self.b1p, self.b2p = dt.type(so.BETA1), dt.type(so.BETA2)
        self.frozen = 0
        self.step = 0

    def set_tables(self, tabs):
        for k, v in tabs.items():
            self.t[k][...] = np.asarray(v, self.dt)

    def forward(self, u, i):
        return forward(self.t, self.indptr, self.items, np.asarray(u, np.int64), np.asarray(i, np.int64), self.item_abs)

    def train_step(self, u, i, r):
        dt = self.dt
        u, i, r = np.asarray(u, np.int64), np.asarray(i, np.int64), np.asarray(r).astype(dt)
        t = self.t
        logits = self.forward(u, i)
        regv = regularizer(t, self.indptr, self.items, u, i, self.reg_bias)
        lossv = so.data_loss(logits, r, self.loss)
        g = so.dlogits(logits, r, self.loss)
        occ = occurrences(t, self.indptr, self.items, u, i, g, self.item_abs, self.reg_bias, self.reg)
        GY, touched = y_gradient(t, self.indptr, self.items, u, occ["W"], occ["c"], occ["users"], self.reg)
        sparse = [(PF, u, occ["P"]), (QF, i, occ["Q"]), (BU, u, occ["bu"]), (BI, i, occ["bi"])]
        if self.optimizer == so.SGD:
            for tid, ids, o in sparse:
                if not (self.frozen >> tid) & 1:
                    so.sgd_sparse(t[tid], ids, o, self.lr)
            if not (self.frozen >> YF) & 1:
                t[YF][touched] -= dt.type(self.lr) * GY[touched]
            if not (self.frozen >> MU) & 1:
                t[MU] -= dt.type(self.lr) * occ["mu"]
        else:
            for tid, ids, o in sparse:
                if (self.frozen >> tid) & 1:
                    continue
                uniq, inv = so.dedup(ids)
                so.adam_sparse_lazy(t[tid], self.slots[tid], uniq, so.segment_sum(o, inv, uniq.size), self.lr,
                                    self.b1p, self.b2p)
            if not (self.frozen >> YF) & 1 and touched.size:
                so.adam_sparse_lazy(t[YF], self.slots[YF], touched, GY[touched], self.lr, self.b1p, self.b2p)
            if not (self.frozen >> MU) & 1:
                so.adam_dense(t[MU], self.slots[MU], occ["mu"], self.lr, self.b1p, self.b2p)
            self.b1p = dt.type(self.b1p * dt.type(so.BETA1))
            self.b2p = dt.type(self.b2p * dt.type(so.BETA2))
        self.step += 1
        return logits, dt.type(lossv), regv
