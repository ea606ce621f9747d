"""Shared helpers of the batched fine-tuning tests (tests/test_finetune_host.py, tests/test_gpu_finetune.py): the float64
oracle behind the calls the drivers make of an SvdModel - the sequential ones (forward, train_steps_repeat) and
finetune_users, executed one user at a time in NumPy with each round's sequential position honoured - and seeded frames."""
import numpy as np

from oracle import svd_oracle as so
from tests.util import make_oracle


def replay_powers(b1p, b2p, b1, b2, n, dtype):
    """the beta powers at steps 0..n of a run, by the oracle's own recurrence (svd_oracle.SvdOracle.train_step)"""
    dt = np.dtype(dtype).type
    out = [(b1p, b2p)]
    for _ in range(n):
        b1p, b2p = dt(b1p * dt(b1)), dt(b2p * dt(b2))
        out.append((b1p, b2p))
    return out


class OracleDriverModel(object):
    """The oracle behind the model interface of tfrecomm_amd.adaptive_test's drivers, sequential and batched."""

    def __init__(self, U, I, D, tables, **kw):
        self.user_num, self.item_num, self.dim = U, I, D
        self.loss = kw.get("loss", "mse")
        self.optimizer = kw.get("optimizer", "adam")
        self.adam_mode = kw.get("adam_mode", "tf1")
        self.o = make_oracle(U, I, D, tables, **kw)
        self.user_order = "reversed"              # finetune_users walks the users in this order: results must not care

    def set_frozen(self, mask):
        self.o.frozen = mask

    def forward(self, u, i):
        return np.asarray(self.o.forward(np.asarray(u, np.int32), np.asarray(i, np.int32)), np.float64)

    def train_steps_repeat(self, u, i, r, nsteps, want_logits=True, want_loss=True):
        u, i, r = np.asarray(u, np.int32), np.asarray(i, np.int32), np.asarray(r, np.float32)
        loss = np.empty(nsteps, np.float64)
        logits = None
        for s in range(nsteps):
            logits, loss[s], _ = self.o.train_step(u, i, r)
        return np.asarray(logits), loss

    def finetune_users(self, users, row_ptr, items, rates, round_ptr, ask_items, prefix_len, nsteps, round_seq=None,
                       want_loss=True, want_final=True):
        o = self.o
        n_rounds = int(round_ptr[-1])
        n_total = n_rounds * nsteps
        seq = np.arange(n_rounds, dtype=np.int64) * nsteps if round_seq is None else np.asarray(round_seq, np.int64)
        adam = o.optimizer == so.ADAM                 # SGD leaves the beta powers where they are
        pw = replay_powers(o.b1p, o.b2p, o.b1 if adam else 1.0, o.b2 if adam else 1.0, n_total, o.dt)
        step0 = o.step
        ask = np.empty(n_rounds, np.float64)
        loss = np.empty(n_rounds, np.float64)
        final = np.full(int(row_ptr[-1]), np.nan, np.float64)
        xs = range(len(users))
        for x in (reversed(xs) if self.user_order == "reversed" else xs):
            u, r0 = int(users[x]), int(row_ptr[x])
            for k in range(int(round_ptr[x]), int(round_ptr[x + 1])):
                ask[k] = self.forward([u], [int(ask_items[k])])[0]
                o.b1p, o.b2p = pw[int(seq[k])]
                n = int(prefix_len[k])
                it = np.asarray(items[r0:r0 + n], np.int32)
                rt = np.asarray(rates[r0:r0 + n], np.float32)
                for s in range(nsteps):
                    logits, loss[k], _ = o.train_step(np.full(n, u, np.int32), it, rt)
                if k + 1 == int(round_ptr[x + 1]):
                    final[r0:r0 + n] = logits
        o.step = step0 + n_total
        o.b1p, o.b2p = pw[n_total]
        return ask, (loss if want_loss else None), (final if want_final else None)

    def user_state(self):
        """user_features, user_bias and (Adam) their slots"""
        o = self.o
        st = [o.P.copy(), o.bu.copy()]
        if o.optimizer == so.ADAM:
            st += [o.slots[so.PF].m.copy(), o.slots[so.PF].v.copy(), o.slots[so.BU].m.copy(), o.slots[so.BU].v.copy()]
        return st


def frame(rs, U, I, n, binary, users=None):
    """a test frame grouped by user, as the reference's (pandas, columns user / item / outcome)"""
    import pandas as pd
    u = np.sort(rs.randint(0, U, n) if users is None else users)
    i = rs.randint(0, I, u.size)
    r = (rs.rand(u.size) < 0.5).astype(np.float32) if binary else rs.randint(1, 6, u.size).astype(np.float32)
    return pd.DataFrame(dict(user=u.astype(np.int32), item=i.astype(np.int32), outcome=r))


def per_user_frame(rs, users, I, per_user, binary, shuffle=True):
    """`per_user` distinct items for each of `users`; rows interleaved across users when `shuffle`"""
    import pandas as pd
    u = np.repeat(np.asarray(users), per_user)
    i = np.concatenate([rs.choice(I, per_user, replace=False) for _ in users])
    r = (rs.rand(u.size) < 0.5).astype(np.float32) if binary else rs.randint(1, 6, u.size).astype(np.float32)
    p = rs.permutation(u.size) if shuffle else np.arange(u.size)
    return pd.DataFrame(dict(user=u[p].astype(np.int32), item=i[p].astype(np.int32), outcome=r[p]))
