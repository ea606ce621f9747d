"""Float64 restatement of the WARP step (include/tfrecomm.h "WARP") on top of tests/bpr_ref.py: the violator
search over ``bpr_ref.candidates``, the weights, the weighted hinge objective, its gradients and a trainer.  NumPy only.

A triple (u, i) walks its candidates c_0 .. c_{attempts-1} in order.  A candidate in row u of the positives is passed over
and not counted; otherwise n += 1 and x = s(u, i) - s(u, c); the first x < margin gives the negative j = c and the trial
count N = n.  No violator: j = -1, N = 0, and the triple is skipped (it contributes nothing and touches nothing).  The
weight is w = log(max(1, (I - 1) // N)).  Per live triple g = -w if x < margin else 0, and the rest is BPR's step."""
import numpy as np

from oracle import svd_oracle as so
from tests import bpr_ref as BR

MU, BU, BI, PF, QF = BR.MU, BR.BU, BR.BI, BR.PF, BR.QF
EPS32 = 2.0 ** -24
BAND = 16                                  # roundings allowed between the float64 x and the device's: see ``examine``


def weights(item_num, trials):
    """w per triple from its trial count N (0 where N = 0)"""
    n = np.asarray(trials, np.int64)
    r = np.maximum(1, (int(item_num) - 1) // np.maximum(n, 1))
    return np.where(n > 0, np.log(r.astype(np.float64)), 0.0)


def examine(t, indptr, items, users, pos, margin, *, seed=0, step=0, attempts=16, item_abs=False):
    """Everything about the search of every triple, [B, attempts] unless said otherwise:
      c      the candidates                        open   c is not a positive of u
      n      open candidates up to and including t  mx     margin - x in float64
      tol    BAND eps32 (sum_d |p| (|q'_i| + |q'_c|) + |bi_i| + |bi_c| + |margin|): what float32 may move margin - x by
             (at most 4 fused terms per lane, 6 butterfly levels, 3 additions: 13 roundings)
      band   open, margin finite and |mx| <= tol: the device may decide either way
      neg, trials [B]   the first open candidate with mx > 0 and its n (-1, 0: none)
      seen   open candidates the reference examines (up to its violator; all of them where there is none)"""
    P, Q, bi = (np.asarray(t[k], np.float64) for k in (PF, QF, BI))
    u, i = np.asarray(users, np.int64), np.asarray(pos, np.int64)
    I = Q.shape[0]
    indptr, items = np.asarray(indptr, np.int64), np.asarray(items, np.int64)
    c = BR.candidates(seed, step, u.size, I, attempts).astype(np.int64)
    keys = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr)) * I + items
    is_open = ~np.isin(u[:, None] * I + c, keys)
    Qt = np.abs(Q) if item_abs else Q
    p = P[u]
    si = np.sum(p * Qt[i], 1) + bi[i]
    x = si[:, None] - (np.einsum("bd,bad->ba", p, Qt[c]) + bi[c])
    X = (np.sum(np.abs(p) * np.abs(Qt[i]), 1) + np.abs(bi[i]))[:, None] + np.einsum("bd,bad->ba", np.abs(p), np.abs(Qt[c])) + np.abs(bi[c])
    with np.errstate(invalid="ignore"):
        mx = margin - x
    tol = BAND * EPS32 * (X + (abs(margin) if np.isfinite(margin) else 0.0))
    band = is_open & (np.abs(mx) <= tol) & bool(np.isfinite(margin))
    n = np.cumsum(is_open, 1)
    viol = is_open & (mx > 0)
    first = np.argmax(viol, 1)
    found = viol.any(1)
    rows = np.arange(u.size)
    neg = np.where(found, c[rows, first], -1)
    trials = np.where(found, n[rows, first], 0)
    seen = is_open & (~found[:, None] | (n <= trials[:, None]))
    return dict(c=c, open=is_open, n=n, mx=mx, tol=tol, band=band, neg=neg, trials=trials, seen=seen)


def search(t, indptr, items, users, pos, margin, **kw):
    """(neg, trials) of every triple"""
    e = examine(t, indptr, items, users, pos, margin, **kw)
    return e["neg"], e["trials"]


def in_band_share(e):
    """share of the triples with a candidate in the band among those the reference examines"""
    return float(np.mean((e["band"] & e["seen"]).any(1)))


def check_search(e, neg, trials):
    """A search's reported (neg, trials) against ``examine``'s ``e``, decisions held outside the band only.  Returns
    (violated statements, share of triples with a band candidate among those the reported search examined).
      - a skipped triple reports N = 0; a live one N >= 1 and its negative is the N-th open candidate
      - an open candidate before the N-th (every one, for a skipped triple) was found not to violate: wrong if mx > tol
      - the N-th was found to violate: wrong if mx < -tol
      - a triple with no band candidate among those the reference examines equals the reference"""
    neg, N = np.asarray(neg, np.int64), np.asarray(trials, np.int64)
    bad = []
    live = neg >= 0
    if ((N > 0) != live).any():
        bad.append("trials: N > 0 on a skipped triple or N = 0 on a live one (%d triples)" % int(((N > 0) != live).sum()))
    nth = e["open"] & (e["n"] == N[:, None]) & live[:, None]
    has = nth.any(1)
    cand = e["c"][np.arange(neg.size), np.argmax(nth, 1)]
    wrong = live & (~has | (cand != neg))
    if wrong.any():
        bad.append("neg: not the N-th open candidate (%d triples, first %d)" % (int(wrong.sum()), int(np.flatnonzero(wrong)[0])))
    passed = e["open"] & (~live[:, None] | (e["n"] < N[:, None]))
    miss = passed & (e["mx"] > e["tol"])
    if miss.any():
        bad.append("search: passed over a candidate that violates the margin beyond the band (%d triples, first %d)"
                   % (int(miss.any(1).sum()), int(np.flatnonzero(miss.any(1))[0])))
    early = nth & (e["mx"] < -e["tol"])
    if early.any():
        bad.append("search: took a candidate that does not violate the margin beyond the band (%d triples, first %d)"
                   % (int(early.any(1).sum()), int(np.flatnonzero(early.any(1))[0])))
    clear = ~(e["band"] & e["seen"]).any(1)
    diff = clear & ((neg != e["neg"]) | (N != e["trials"]))
    if diff.any():
        bad.append("search: a triple with no candidate in the band differs from the reference (%d triples, first %d)"
                   % (int(diff.sum()), int(np.flatnonzero(diff)[0])))
    share = float(np.mean((e["band"] & (passed | nth)).any(1)))
    return bad, share


def _live(u, i, j, w):
    keep = np.asarray(j) >= 0
    return tuple(np.asarray(a, dt)[keep] for a, dt in ((u, np.int64), (i, np.int64), (j, np.int64), (w, np.float64)))


def terms(t, u, i, j, w, margin, item_abs=False, reg_bias=False):
    """(x, data, reg) over the live triples: data = sum w max(0, margin - x)"""
    u, i, j, w = _live(u, i, j, w)
    P, Q, bi = t[PF], t[QF], t[BI]
    Qt = np.abs(Q) if item_abs else Q
    x = (np.sum(P[u] * Qt[i], 1) + bi[i]) - (np.sum(P[u] * Qt[j], 1) + bi[j])
    data = np.sum(w * np.maximum(0.0, margin - x))
    reg = 0.5 * np.sum(np.sum(P[u] ** 2, 1) + np.sum(Q[i] ** 2, 1) + np.sum(Q[j] ** 2, 1))
    if reg_bias:
        reg += 0.5 * np.sum(bi[i] ** 2 + bi[j] ** 2)
    return x, data, reg


def cost(t, u, i, j, w, margin, lam, item_abs=False, reg_bias=False):
    """the objective whose gradient a step takes with (j, w) held fixed"""
    _, data, reg = terms(t, u, i, j, w, margin, item_abs, reg_bias)
    return data + lam * reg


def gradients(t, u, i, j, w, margin, lam, item_abs=False, reg_bias=False):
    """dense d cost / d table for BI, PF, QF, and the touched rows of each: {id: (grad, touched bool mask)}"""
    u, i, j, w = _live(u, i, j, w)
    P, Q, bi = t[PF], t[QF], t[BI]
    Qt = np.abs(Q) if item_abs else Q
    sg = np.sign(Q) if item_abs else np.ones_like(Q)
    x = (np.sum(P[u] * Qt[i], 1) + bi[i]) - (np.sum(P[u] * Qt[j], 1) + bi[j])
    g = np.where(x < margin, -w, 0.0).astype(P.dtype)
    dP, dQ, dbi = np.zeros_like(P), np.zeros_like(Q), np.zeros_like(bi)
    np.add.at(dP, u, g[:, None] * (Qt[i] - Qt[j]) + lam * P[u])
    np.add.at(dQ, i, g[:, None] * P[u] * sg[i] + lam * Q[i])
    np.add.at(dQ, j, -g[:, None] * P[u] * sg[j] + lam * Q[j])
    np.add.at(dbi, i, g + (lam * bi[i] if reg_bias else 0.0))
    np.add.at(dbi, j, -g + (lam * bi[j] if reg_bias else 0.0))
    tu = np.zeros(P.shape[0], bool)
    tu[u] = True
    ti = np.zeros(Q.shape[0], bool)
    ti[i] = True
    ti[j] = True
    return {PF: (dP, tu), QF: (dQ, ti), BI: (dbi, ti)}


class WarpRef(BR.BprRef):
    """The WARP step on the SVD model's tables in float64: the search on the pre-step tables, then BPR's update rules."""

    def __init__(self, U, I, D, *, margin=1.0, seed=0, attempts=16, **kw):
        super().__init__(U, I, D, **kw)
        self.margin, self.seed, self.attempts = float(margin), seed, attempts
        self.indptr = self.items = None

    def set_positives(self, indptr, items):
        self.indptr, self.items = np.asarray(indptr, np.int64), np.asarray(items, np.int64)

    def train_step(self, u, i, j=None):
        """returns (neg, trials, data, reg)"""
        t, dt = self.t, self.dt
        I = t[QF].shape[0]
        if j is None:
            j, trials = search(t, self.indptr, self.items, u, i, self.margin, seed=self.seed, step=self.step,
                               attempts=self.attempts, item_abs=self.item_abs)
        else:
            j, trials = np.asarray(j, np.int64), np.ones(np.size(j), np.int64)
        w = weights(I, trials)
        _, data, reg = terms(t, u, i, j, w, self.margin, self.item_abs, self.reg_bias)
        G = gradients(t, u, i, j, w, self.margin, dt.type(self.reg), self.item_abs, self.reg_bias)
        for k, (g, touched) in G.items():
            if (self.frozen >> k) & 1:
                continue
            rows = np.flatnonzero(touched)
            if self.optimizer == "sgd":
                t[k][rows] -= dt.type(self.lr) * g[rows]
            elif rows.size:
                so.adam_sparse_lazy(t[k], self.slots[k], rows, g[rows], self.lr, self.b1p, self.b2p)
        if self.optimizer != "sgd":
            self.b1p = dt.type(self.b1p * dt.type(so.BETA1))
            self.b2p = dt.type(self.b2p * dt.type(so.BETA2))
        self.step += 1
        return j, trials, data, reg
