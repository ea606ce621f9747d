"""Float64 restatement of the BPR step (include/tfrecomm.h "BPR") and its negative sampler in NumPy uint64.

A triple (u, i, j) with j = -1 is skipped: it contributes nothing and touches nothing.  Tables are a dict keyed by the
C-ABI's table ids (MU, BU, BI, PF, QF); a BPR step reads and writes BI, PF and QF only."""
import numpy as np

from oracle import svd_oracle as so

MU, BU, BI, PF, QF = so.MU, so.BU, so.BI, so.PF, so.QF
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def mix(z):
    """splitmix64's finaliser, elementwise on uint64 (wraps mod 2^64)"""
    z = np.asarray(z, np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def step_key(seed, step):
    return mix(mix(np.uint64(seed) ^ GOLDEN) ^ np.uint64(step & 0xFFFFFFFFFFFFFFFF))


def candidates(seed, step, batch, item_num, attempts):
    """[batch, attempts] draws j_a of every position b"""
    k = step_key(seed, step)
    b = np.arange(batch, dtype=np.uint64)[:, None]
    a = np.arange(attempts, dtype=np.uint64)[None, :]
    r = mix(k ^ ((b << np.uint64(6)) | a))
    return ((r >> np.uint64(32)) * np.uint64(item_num)) >> np.uint64(32)


def sample(indptr, items, users, item_num, seed=0, step=0, attempts=16):
    """the first draw of each position that is not a positive of its user (binary search of the row), else -1"""
    users = np.asarray(users, np.int64)
    c = candidates(seed, step, users.size, item_num, attempts).astype(np.int64)
    out = np.full(users.size, -1, np.int64)
    for b, u in enumerate(users):
        row = np.asarray(items[int(indptr[u]):int(indptr[u + 1])], np.int64)
        for j in c[b]:
            p = np.searchsorted(row, j)
            if p == row.size or row[p] != j:
                out[b] = j
                break
    return out


def terms(t, u, i, j, item_abs=False, reg_bias=False):
    """(x, data, reg) over the triples that are not skipped"""
    keep = np.asarray(j) >= 0
    u, i, j = (np.asarray(a, np.int64)[keep] for a in (u, i, j))
    P, Q, bi = t[PF], t[QF], t[BI]
    Qt = np.abs(Q) if item_abs else Q
    x = (np.sum(P[u] * Qt[i], 1) + bi[i]) - (np.sum(P[u] * Qt[j], 1) + bi[j])
    data = np.sum(np.logaddexp(0.0, -x))
    reg = 0.5 * np.sum(np.sum(P[u] ** 2, 1) + np.sum(Q[i] ** 2, 1) + np.sum(Q[j] ** 2, 1))
    if reg_bias:
        reg += 0.5 * np.sum(bi[i] ** 2 + bi[j] ** 2)
    return x, data, reg


def cost(t, u, i, j, lam, item_abs=False, reg_bias=False):
    _, data, reg = terms(t, u, i, j, item_abs, reg_bias)
    return data + lam * reg


def gradients(t, u, i, j, lam, item_abs=False, reg_bias=False):
    """dense d cost / d table for BI, PF, QF, and the touched rows of each: {id: (grad, touched bool mask)}"""
    keep = np.asarray(j) >= 0
    u, i, j = (np.asarray(a, np.int64)[keep] for a in (u, i, j))
    P, Q, bi = t[PF], t[QF], t[BI]
    Qt = np.abs(Q) if item_abs else Q
    sg = np.sign(Q) if item_abs else np.ones_like(Q)
    x = (np.sum(P[u] * Qt[i], 1) + bi[i]) - (np.sum(P[u] * Qt[j], 1) + bi[j])
    g = -1.0 / (1.0 + np.exp(x))                                       # -sigmoid(-x)
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


class BprRef:
    """The BPR step on the SVD model's tables: SGD or lazy Adam on the touched rows, frozen bits BI / PF / QF."""

    def __init__(self, U, I, D, *, item_abs=False, reg_bias=False, optimizer="adam", lr=1e-3, reg=0.05,
                 dtype=np.float64):
        self.dt = np.dtype(dtype)
        dt = self.dt
        self.item_abs, self.reg_bias, self.optimizer = bool(item_abs), bool(reg_bias), optimizer
        self.lr, self.reg = lr, reg
        self.t = {MU: np.zeros((), dt), BU: np.zeros(U, dt), BI: np.zeros(I, dt), PF: np.zeros((U, D), dt),
                  QF: np.zeros((I, D), dt)}
        self.slots = {k: so.AdamState(v.shape, dt) for k, v in self.t.items()}
        self.b1p, self.b2p = dt.type(so.BETA1), dt.type(so.BETA2)
        self.frozen = 0
        self.step = 0

    def set_tables(self, tabs):
        for k, v in tabs.items():
            self.t[k][...] = np.asarray(v, self.dt)

    def train_step(self, u, i, j):
        t, dt = self.t, self.dt
        _, data, reg = terms(t, u, i, j, self.item_abs, self.reg_bias)
        G = gradients(t, u, i, j, dt.type(self.reg), self.item_abs, self.reg_bias)
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
        return data, reg


def auc(t, users, pos_csr, excl_csr, item_abs=False):
    """mean over users with held-out items of P(score(held-out) > score(non-positive)), ties 1/2 (float64 scores)"""
    P, Q, bi = t[PF], t[QF], t[BI]
    Qt = np.abs(Q) if item_abs else Q
    out = []
    for u in users:
        tgt = pos_csr[u]
        if tgt.size == 0:
            continue
        s = P[u] @ Qt.T + bi
        elig = np.ones(Q.shape[0], bool)
        elig[excl_csr[u]] = False
        elig[tgt] = False
        neg = np.sort(s[elig])
        st = s[tgt]
        lo = np.searchsorted(neg, st, "left")
        hi = np.searchsorted(neg, st, "right")
        out.append(np.mean((lo + 0.5 * (hi - lo)) / max(neg.size, 1)))
    return float(np.mean(out))
