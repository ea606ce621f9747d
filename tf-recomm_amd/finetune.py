"""Batched per-user fine-tuning: every user of the drivers in tfrecomm_amd.adaptive_test in ONE library call.

`adaptive_test.non_adaptive_test` / `adaptive_test.adaptive_test` (reference non_adaptive_test.py, adaptive_test.py) walk the
test users one after another, one `tfr_train_steps_repeat` per round.  With mu and the item tables frozen (`FROZEN_BUT_USER`,
what both drivers set) and SGD or lazy Adam, one user's rounds read the frozen item side and write only that user's row,
bias and slots, so the users are independent chains: `SvdModel.finetune_users` runs them all in one launch, one wave per
user (csrc/finetune.hip).

A driver run reduces to a `Schedule` (built and validated here, before any device work): per user its training rows, and
per round the asked item, the number of rows it trains on and the step at which the sequential driver would start it (lazy
Adam's lr_t depends on the global step).  `non_adaptive_test` / `adaptive_test` below take the sequential drivers' arguments
plus `batched`: with `batched=True` they make that one call and return the sequential drivers' structures, calling `log`
afterwards once per round in the sequential order; with `batched=False` (the default) they ARE the sequential drivers.
The batched sums run in another order than the sequential steps, so its numbers match them to float32 rounding, not bit
for bit; that is why the default stays sequential (the sequential drivers are bit-identical to the reference's own
`sess.run` spelling, tests/test_adaptive.py).
"""
import numpy as np

from . import _lib as L
from . import adaptive_test as _seq
from . import cats
from .adaptive_test import FROZEN_BUT_USER, _columns, _head, roc_auc
from .ops import sigmoid

__all__ = ["Schedule", "non_adaptive_schedule", "adaptive_schedule", "non_adaptive_test", "adaptive_test",
           "FROZEN_BUT_USER"]


def _columns_by_user(users):
    """(user ids in first-appearance order, row_ptr, rows of `users` grouped by those users, each group in frame order)"""
    if users.size == 0:
        return np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64)
    uniq, first, inv = np.unique(users, return_index=True, return_inverse=True)
    rank = np.empty(uniq.size, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(uniq.size)
    slot = rank[inv.reshape(-1)]
    order = np.argsort(slot, kind="stable")
    row_ptr = np.concatenate(([0], np.cumsum(np.bincount(slot, minlength=uniq.size)))).astype(np.int64)
    return users[np.sort(first)], row_ptr, order


class Schedule(object):
    """Every round of a driver run, grouped by user (the argument of `SvdModel.finetune_users`).  User `users[x]` trains on
    rows [row_ptr[x], row_ptr[x+1]) of items / rates; its rounds are [round_ptr[x], round_ptr[x+1]): round k predicts
    ask[k] with the parameters of the moment, then trains `nsteps` steps on the user's first prefix[k] rows.  seq[k] is the
    step, counted from the run's start, at which the sequential driver starts round k (what lazy Adam's lr_t depends on)."""

    def __init__(self, users, row_ptr, items, rates, round_ptr, ask, prefix, seq, nsteps):
        self.users = np.asarray(users, np.int64)
        self.row_ptr = np.asarray(row_ptr, np.int64)
        self.items = np.asarray(items, np.int64)
        self.rates = np.asarray(rates, np.float32)
        self.round_ptr = np.asarray(round_ptr, np.int64)
        self.ask = np.asarray(ask, np.int64)
        self.prefix = np.asarray(prefix, np.int32)
        self.seq = np.asarray(seq, np.int64)
        self.nsteps = int(nsteps)

    @property
    def n_rounds(self):
        return int(self.round_ptr[-1])

    def validate(self, user_num, item_num):
        """Everything `tfr_finetune_users` checks, raised here before any device work: ValueError for the shape,
        OutOfRangeError (an IndexError) for ids."""
        n = self.users.size
        if self.row_ptr.shape != (n + 1,) or self.round_ptr.shape != (n + 1,):
            raise ValueError("schedule: row_ptr and round_ptr must hold n_users + 1 offsets")
        if self.row_ptr[0] != 0 or self.round_ptr[0] != 0 or np.any(np.diff(self.row_ptr) < 0) or np.any(np.diff(self.round_ptr) < 0):
            raise ValueError("schedule: offsets must start at 0 and be monotone")
        nr, nk = int(self.row_ptr[-1]), int(self.round_ptr[-1])
        if self.items.shape != (nr,) or self.rates.shape != (nr,):
            raise ValueError("schedule: items / rates must hold row_ptr[-1] entries")
        if self.ask.shape != (nk,) or self.prefix.shape != (nk,) or self.seq.shape != (nk,):
            raise ValueError("schedule: ask / prefix / seq must hold round_ptr[-1] entries")
        if self.nsteps < 1:
            raise ValueError("schedule: at least one training step per round")
        if n and (self.users.min() < 0 or self.users.max() >= user_num):
            raise L.OutOfRangeError(L.ERR_OOB, "schedule: user id outside [0, %d)" % user_num)
        for what, ids in (("item", self.items), ("asked item", self.ask)):
            if ids.size and (ids.min() < 0 or ids.max() >= item_num):
                raise L.OutOfRangeError(L.ERR_OOB, "schedule: %s id outside [0, %d)" % (what, item_num))
        if np.unique(self.users).size != n:
            raise ValueError("schedule: a user appears more than once")
        rows_of_round = np.repeat(np.diff(self.row_ptr), np.diff(self.round_ptr))
        if np.any(self.prefix < 1) or np.any(self.prefix > rows_of_round):
            raise ValueError("schedule: every round must train on 1 .. (its user's rows) rows")
        if nk and (self.seq.min() < 0 or self.seq.max() > (nk - 1) * self.nsteps):
            raise ValueError("schedule: round positions outside the run's steps")
        return self


def non_adaptive_schedule(test, epoch_max=100, max_user=None):
    """The schedule of `non_adaptive_test`: rows up to the first one whose user exceeds `max_user`, grouped by user in
    frame order; a round per row (ask = the row's item, trained on the user's rows up to it), started at row index x
    epoch_max.  Also returns, per kept row in frame order, the index of its round."""
    users, items, outcomes = _columns(test)
    keep = users.size
    if max_user is not None:
        over = np.nonzero(users > max_user)[0]
        if over.size:
            keep = int(over[0])
    users, items, outcomes = users[:keep], items[:keep], outcomes[:keep]
    uid, row_ptr, order = _columns_by_user(users)
    counts = np.diff(row_ptr)
    prefix = np.arange(keep, dtype=np.int64) - np.repeat(row_ptr[:-1], counts) + 1
    round_of_row = np.empty(keep, np.int64)
    round_of_row[order] = np.arange(keep)
    sched = Schedule(uid, row_ptr, items[order], outcomes[order], row_ptr, items[order], prefix,
                     order.astype(np.int64) * epoch_max, epoch_max)
    return sched, round_of_row


def adaptive_schedule(test, budget=10, epoch_max=300, selector=cats.Next, max_users=3, ask_everything=False,
                      popularity=None):
    """The schedule of `adaptive_test`.  The selectors do not look at the model, so the asked items are drawn here, user by
    user and round by round as the sequential driver draws them (cats.Random consumes Python's `random` in the same
    order).  Rows: the asked items with their outcomes (first matching row), or the user's whole test set with
    `ask_everything`; round b of user x trains on b + 1 rows (all of them with `ask_everything`), started at
    (x * budget + b) x epoch_max.  Raises ValueError for a user with fewer than `budget` test items before anything is
    drawn.  Also returns, per user, its rows' outcomes as the driver's `outcome` list."""
    users, items, outcomes = _columns(test)
    uid, row_ptr, order = _columns_by_user(users)
    nu = min(uid.size, max_users) if max_users is not None else uid.size
    for x in range(nu):
        n = int(row_ptr[x + 1] - row_ptr[x])
        if n < budget:
            raise ValueError("user %d has %d test items, fewer than the budget of %d" % (uid[x], n, budget))
    s_items, s_rates, s_ptr, ask, prefix, outcome = [], [], [0], [], [], []
    for x in range(nu):
        rows = order[row_ptr[x]:row_ptr[x + 1]]
        t_items, t_rates = items[rows], outcomes[rows]
        cat = selector(t_items, popularity) if selector is cats.Popular else selector(t_items)
        asked = [cat.next_item() for _ in range(budget)]
        rates = [float(t_rates[np.nonzero(t_items == item)[0][0]]) for item in asked]
        outcome.append(rates)
        ask.extend(asked)
        if ask_everything:
            s_items.append(t_items); s_rates.append(t_rates)
            prefix.extend([t_items.size] * budget)
        else:
            s_items.append(np.asarray(asked, np.int64)); s_rates.append(np.asarray(rates, np.float32))
            prefix.extend(range(1, budget + 1))
        s_ptr.append(s_ptr[-1] + s_items[-1].size)
    cat_ = (lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt))
    sched = Schedule(uid[:nu], s_ptr, cat_(s_items, np.int64), cat_(s_rates, np.float32), np.arange(nu + 1) * budget,
                     ask, prefix, np.arange(nu * budget, dtype=np.int64) * epoch_max, epoch_max)
    return sched, outcome


def _check_batchable(model, freeze):
    if not freeze:
        raise ValueError("batched=True needs freeze=True: with the item tables and mu training, every user's steps move "
                         "rows the other users read, so the users cannot run side by side")
    if getattr(model, "optimizer", None) == "adam" and getattr(model, "adam_mode", None) == "tf1":
        raise ValueError("batched=True needs SGD or lazy Adam: tf1-mode Adam decays and moves every user row at every "
                         "step, which couples the users")


def _run(model, sched, want_loss):
    sched.validate(model.user_num, model.item_num)
    model.set_frozen(FROZEN_BUT_USER)
    return model.finetune_users(sched.users, sched.row_ptr, sched.items, sched.rates, sched.round_ptr, sched.ask,
                                sched.prefix, sched.nsteps, round_seq=sched.seq, want_loss=want_loss, want_final=True)


def non_adaptive_test(model, test, epoch_max=100, max_user=None, freeze=True, log=None, batched=False):
    """`adaptive_test.non_adaptive_test` (non_adaptive_test.py:56-121), every user in one library call with `batched=True`:
    same dict (accuracy, auc, truth, pred), `log` called per row in frame order afterwards.  Raises ValueError, before
    touching the model, when the run cannot be batched (freeze=False, tf1 Adam)."""
    if not batched:
        return _seq.non_adaptive_test(model, test, epoch_max=epoch_max, max_user=max_user, freeze=freeze, log=log)
    _check_batchable(model, freeze)
    sched, round_of_row = non_adaptive_schedule(test, epoch_max, max_user)
    ask_logits, loss, _ = _run(model, sched, want_loss=log is not None)
    proba = sigmoid(np.asarray(ask_logits)[round_of_row])
    truth = [float(x) for x in sched.rates[round_of_row]]
    pred = [float(x) for x in proba]
    if log is not None:
        users = np.repeat(sched.users, np.diff(sched.round_ptr))
        for r, k in enumerate(round_of_row.tolist()):
            log(dict(user=int(users[k]), item=int(sched.ask[k]), outcome=truth[r], predicted=pred[r],
                     history=int(sched.prefix[k]), last_cost=float(loss[k])))
    truth_a, pred_a = np.asarray(truth, np.float32), np.asarray(pred, np.float64)
    return dict(accuracy=float(np.mean(np.round(pred_a) == truth_a)) if truth else float("nan"),
                auc=roc_auc(truth_a, pred_a), truth=truth, pred=pred)


def adaptive_test(model, test, budget=10, epoch_max=300, selector=cats.Next, max_users=3, ask_everything=False,
                  popularity=None, freeze=True, log=None, batched=False):
    """`adaptive_test.adaptive_test` (adaptive_test.py:54-127), every user in one library call with `batched=True`: same
    records (user, asked, predicted, outcome, size, macc, mobo, rmse, mcost), `log` called per round afterwards.
    `max_users=None` takes every user.  Raises ValueError, before touching the model, when the run cannot be batched
    (freeze=False, tf1 Adam) or a user has fewer than `budget` test items."""
    if not batched:
        return _seq.adaptive_test(model, test, budget=budget, epoch_max=epoch_max, selector=selector, max_users=max_users,
                                  ask_everything=ask_everything, popularity=popularity, freeze=freeze, log=log)
    _check_batchable(model, freeze)
    sched, outcome = adaptive_schedule(test, budget, epoch_max, selector, max_users, ask_everything, popularity)
    ask_logits, loss, final = _run(model, sched, want_loss=True)
    proba = sigmoid(np.asarray(ask_logits))
    out = []
    for x in range(sched.users.size):
        k0, k1, r0 = int(sched.round_ptr[x]), int(sched.round_ptr[x + 1]), int(sched.row_ptr[x])
        size = int(sched.prefix[k1 - 1])
        rec = dict(user=int(sched.users[x]), asked=[int(i) for i in sched.ask[k0:k1]],
                   predicted=[float(p) for p in proba[k0:k1]], outcome=outcome[x])
        if log is not None:
            for b in range(k1 - k0):
                log(dict(user=rec["user"], budget=b, item=rec["asked"][b], predicted=rec["predicted"][b],
                         outcome=rec["outcome"][b]))
        infer = _head(model, final[r0:r0 + size])
        tr = sched.rates[r0:r0 + size]
        rec.update(size=size, macc=float(np.mean(infer == tr)), mobo=float(np.mean(np.abs(infer - tr) <= 1)),
                   rmse=float(np.sqrt(np.mean((infer - tr) ** 2))), mcost=float(loss[k1 - 1]))
        out.append(rec)
    return out
