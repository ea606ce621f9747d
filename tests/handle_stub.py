"""A NumPy stand-in for the part of ``SvdModel`` that tests/handle_states.py drives, so that the call-sequence harness itself
runs where there is no GPU (tests/test_call_sequence_host.py).  The arithmetic is the float32 oracle's (oracle/svd_oracle.py),
which keeps no state besides tables, slots and counters: long-lived and fresh stand-ins agree bit for bit by construction.

``defect`` plants the kinds of fault the harness exists to find, each a piece of left-behind state that one reader forgets:
  "stale_forward"   forward reads item rows as they were at the last get_table / set_table (a missing settle);
  "kept_sort"       the last staged step of a call gathers and sorts the batch that follows; a new store does not void it
                    (a published look-ahead sort that survives);
  "run_ahead"       draw_ids forgets to cancel the run-ahead: it continues the generator from behind the ids drawn ahead."""
import numpy as np

from oracle import svd_oracle as so
from tests import step_cases as SC
from tests.handle_states import plan_word

SLOT_M, SLOT_V = 8, 16


class StubModel(object):
    def __init__(self, user_num, item_num, dim, *, loss="mse", item_abs=False, reg_bias=False, optimizer="adam", adam_mode="tf1",
                 lr=1e-3, reg=0.05, defect=None, **_):
        self.U, self.I, self.D = user_num, item_num, dim
        self.opt, self.mode, self.defect = optimizer, adam_mode, defect
        self.o = so.SvdOracle(user_num, item_num, dim, loss=so.NLL if loss == "nll" else so.MSE, item_abs=item_abs, reg_bias=reg_bias,
                              optimizer=so.SGD if optimizer == "sgd" else so.ADAM, adam_mode=so.TF1 if adam_mode == "tf1" else so.LAZY,
                              lr=lr, reg=reg, dtype=np.float32)
        self.o.set_tables(0, 0, 0, 0, 0)
        self.rs = None
        self.store = self.evalset = self.staged = None
        self._q_seen = None                              # stale_forward: item rows as the last settle saw them
        self._ahead = None                               # run_ahead: (generator state before the ids drawn ahead, B)
        self._kept = None                                # kept_sort: the batch sorted ahead by the last staged step

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def close(self):
        pass

    # -- variables
    def _arr(self, which):
        t = which & 7
        if which & SLOT_M:
            return self.o.slots[t].m
        if which & SLOT_V:
            return self.o.slots[t].v
        return self.o.tables()[t]

    def get_table(self, which):
        self._q_seen = None
        return np.array(self._arr(which), np.float32)

    def set_table(self, which, values):
        self._q_seen = None
        a = self._arr(which)
        a[...] = np.asarray(values, np.float32).reshape(a.shape)

    def set_tables(self, mu, bu, bi, P, Q):
        for which, x in enumerate((mu, bu, bi, P, Q)):
            self.set_table(which, x)

    def init_tables(self, seed=0, feature_stddev=0.02, bias_stddev=1.0):
        rs = np.random.RandomState(seed)
        self.set_tables(rs.uniform(-1, 1), rs.normal(0, bias_stddev, self.U), rs.normal(0, bias_stddev, self.I),
                        rs.normal(0, feature_stddev, (self.U, self.D)), rs.normal(0, feature_stddev, (self.I, self.D)))
        self.o.reset_optimizer()
        self.o.step = 0

    def set_frozen(self, mask):
        self.o.frozen = int(mask)

    def set_hyper(self, lr, reg):
        self.o.lr, self.o.reg = lr, reg

    def get_step(self):
        return self.o.step, float(self.o.b1p), float(self.o.b2p)

    def set_step(self, step, b1p, b2p):
        self.o.step, self.o.b1p, self.o.b2p = int(step), np.float32(b1p), np.float32(b2p)

    def kernel_plan(self, batch):
        return {"plan": plan_word(SC.path_of(self.U, self.I, batch, self.opt, self.mode))}

    def sync(self):
        pass

    # -- forward, evaluation, steps
    def forward(self, users, items):
        if self.defect == "stale_forward" and self._q_seen is not None:
            q, self.o.Q = self.o.Q, self._q_seen
            try:
                return np.asarray(self.o.forward(users, items), np.float32)
            finally:
                self.o.Q = q
        return np.asarray(self.o.forward(users, items), np.float32)

    def eval(self, users, items, rates):
        inf = np.asarray(self.o.infer(users, items), np.float32)
        r = np.asarray(rates, np.float32)
        return float(np.sum((inf.astype(np.float64) - r) ** 2)), int(np.sum(inf == r))

    def train_step(self, users, items, rates, want_logits=True):
        if self.defect == "stale_forward" and self._q_seen is None:
            self._q_seen = self.o.Q.copy()               # the rows this step moves "to the other table": forward will not look there
        lg, loss, reg = self.o.train_step(users, items, rates)
        return (np.asarray(lg, np.float32) if want_logits else None), float(loss), float(reg)

    def train_steps_repeat(self, users, items, rates, nsteps, want_logits=True, want_loss=True):
        loss = np.empty(nsteps, np.float32)
        for s in range(nsteps):
            lg, loss[s], _ = self.train_step(users, items, rates)
        return lg, loss

    # -- resident store
    def upload_triples(self, users, items, rates):
        self.store = (np.asarray(users), np.asarray(items), np.asarray(rates))
        self._cancel()
        if self.defect != "kept_sort":
            self._kept = None

    def upload_eval_triples(self, users, items, rates):
        self.evalset = (users, items, rates)

    def eval_resident(self):
        return self.eval(*self.evalset) + (len(self.evalset[0]),)

    def forward_resident(self, lo, hi):
        return self.forward(self.store[0][lo:hi], self.store[1][lo:hi])

    def _rows(self, ids):
        return tuple(c[ids] for c in self.store)

    def _on_ids(self, ids):
        return self.train_step(*self._rows(ids))[1]

    def stage_ids(self, ids):
        self.staged = np.array(ids, np.int64)
        self._kept = None

    def staged_ids_devptr(self):
        return 0, 0 if self.staged is None else self.staged.size

    def train_steps_staged(self, first_step, batch, nsteps, want_loss=False):
        loss = np.empty(nsteps, np.float32)
        for s in range(nsteps):
            k0 = (first_step + s) * batch
            rows = self._rows(self.staged[k0:k0 + batch])
            if s == 0 and self._kept is not None and self._kept[0] == (k0, batch):
                rows = self._kept[1]                     # gathered ahead: only the kept_sort defect leaves stale rows here
            self._kept = None
            loss[s] = self.train_step(*rows)[1]
        k0 = (first_step + nsteps) * batch
        self._kept = ((k0, batch), self._rows(self.staged[k0:k0 + batch])) if k0 + batch <= self.staged.size else None
        return loss if want_loss else None

    def train_steps_resident(self, ids, batch, want_loss=True):
        self.stage_ids(ids)
        return self.train_steps_staged(0, batch, np.asarray(ids).size // batch, want_loss)

    def train_step_ids(self, ids):
        self._kept = None
        self._on_ids(np.asarray(ids, np.int64))

    # -- the id draw, with a run-ahead that every other reader of the generator must cancel
    def _cancel(self):
        if self._ahead is not None:
            self.rs.set_state(self._ahead[0])
            self._ahead = None

    def rng_seed(self, seed):
        self.rs, self._ahead = np.random.RandomState(seed), None

    def rng_set_state(self, key, pos):
        self.rs = np.random.RandomState(0)
        self.rs.set_state(("MT19937", np.asarray(key, np.uint32), int(pos), 0, 0.0))
        self._ahead = None

    def rng_get_state(self):
        self._cancel()
        st = self.rs.get_state()
        return np.array(st[1], np.uint32), int(st[2])

    def rng_to_numpy(self):
        k, pos = self.rng_get_state()
        st = np.random.get_state()
        np.random.set_state((st[0], k, pos, st[3], st[4]))

    def rng_from_numpy(self):
        st = np.random.get_state()
        self.rng_set_state(st[1], st[2])

    def draw_ids(self, high, count):
        if self.defect != "run_ahead":
            self._cancel()
        return self.rs.randint(0, high, count).astype(np.int64)

    def train_steps_drawn(self, batch, nsteps, want_loss=False):
        N = self.store[0].size
        if self._ahead is not None and self._ahead[1] != batch:
            self._cancel()
        if self._ahead is not None:
            self.rs.set_state(self._ahead[0])            # the ids drawn ahead are this call's first: the same stream either way
            self._ahead = None
        self._kept = None
        loss = np.array([self._on_ids(self.rs.randint(0, N, batch)) for _ in range(nsteps)], np.float32)
        self._ahead = (self.rs.get_state(), batch)
        self.rs.randint(0, N, batch)                     # the next call's first batch, drawn ahead
        return loss if want_loss else None
