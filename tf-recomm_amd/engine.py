"""SvdModel: thin object wrapper over the C-ABI handle (include/tfrecomm.h).

Holds no arithmetic: every number comes from the HIP kernels.  The reference-shaped
surface (``ops.inference_svd`` / ``ops.optimization`` / ``Session.run``) in ``ops.py``
and ``graph.py`` is built on this class.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def device_copy_rate(device=0, nbytes=1 << 30, reps=10):
    """(best, mean) GB/s (read + write) of the library's own float4 copy kernel - bench.py's same-device yardstick."""
    lib = L.load()
    best, mean = C.c_double(), C.c_double()
    L.check(lib.tfr_device_copy_rate(int(device), int(nbytes), int(reps), C.byref(best), C.byref(mean)))
    return best.value, mean.value


def rated_matrix(user_ids, item_ids, user_num, item_num):
    """The rated pairs of training columns (e.g. a ``dataio`` frame's ``user`` / ``item``) as a ``scipy.sparse`` CSR
    ``[user_num, item_num]``: row ``u`` lists, sorted and without repeats, the items ``u`` rated - the ``exclude``
    argument of ``SvdModel.recommend``."""
    import scipy.sparse as sp
    u = np.asarray(L.as_i32(user_ids, "user ids"), np.int64).reshape(-1)
    i = np.asarray(L.as_i32(item_ids, "item ids"), np.int64).reshape(-1)
    if u.shape != i.shape:
        raise ValueError("user and item columns must have equal length")
    if u.size and (u.min() < 0 or u.max() >= user_num or i.min() < 0 or i.max() >= item_num):
        raise L.OutOfRangeError(L.ERR_OOB, "ids outside [0, %d) x [0, %d)" % (user_num, item_num))
    x = sp.csr_matrix((np.ones(u.size, np.float32), (u, i)), shape=(int(user_num), int(item_num)))
    x.sum_duplicates()                                 # also sorts each row
    return x


def exclusion_csr(exclude, rows):
    """``exclude`` as the C-ABI's (indptr int64, items int32) aligned with ``rows``, or (None, None).  ``exclude`` is None,
    an (indptr, indices) pair already aligned with ``rows``, or a ``scipy.sparse`` matrix whose row ``r`` lists what to
    exclude for id ``r`` (gathered for ``rows`` and sorted here)."""
    if exclude is None:
        return None, None
    if isinstance(exclude, tuple):
        indptr, items = exclude
        indptr = np.ascontiguousarray(np.asarray(indptr, np.int64)).reshape(-1)
        items = L.as_i32(items, "excluded items").reshape(-1)
        if indptr.size != len(rows) + 1:
            raise ValueError("exclusion indptr must hold n_users + 1 entries")
        if indptr.size and indptr[-1] > items.size:
            raise ValueError("exclusion indptr points past its items")
        return indptr, items
    x = exclude.tocsr()[np.asarray(rows, np.int64)]
    x.sort_indices()
    return np.ascontiguousarray(x.indptr, np.int64), np.ascontiguousarray(x.indices, np.int32)


def target_csr(targets, rows):
    """``targets`` as the C-ABI's target rows: (indptr int64 from 0, items int32 with every row strictly increasing, order).
    ``targets`` is an (indptr, items) pair aligned with ``rows`` (a row in any order; ``order`` is the permutation that sorted
    it: sorted position ``j`` holds the caller's item ``order[j]``; None when the rows were already strictly increasing) or a
    ``scipy.sparse`` matrix whose row ``r`` lists the targets of id ``r`` (gathered for ``rows``; ``order`` None, the ranks
    follow the gathered rows' sorted indices).
    A repeated item in a row raises ValueError."""
    if isinstance(targets, tuple):
        indptr, items = targets
        indptr = np.asarray(indptr, np.int64).reshape(-1)
        items = L.as_i32(items, "target items").reshape(-1)
        if indptr.size != len(rows) + 1:
            raise ValueError("target indptr must hold n_users + 1 entries")
        if indptr.size and (indptr[0] < 0 or np.any(np.diff(indptr) < 0) or indptr[-1] > items.size):
            raise ValueError("target indptr must be non-decreasing and inside its items")
        items = items[indptr[0]:indptr[-1]]
        indptr = indptr - indptr[0]
        row = np.repeat(np.arange(len(rows), dtype=np.int64), np.diff(indptr))
        order = None
        if items.size > 1 and np.any((items[1:] <= items[:-1]) & (row[1:] == row[:-1])):
            order = np.lexsort((items, row))           # rows not yet strictly increasing: sort them, remember how
            items = np.ascontiguousarray(items[order])
    else:
        x = targets.tocsr()[np.asarray(rows, np.int64)]
        x.sort_indices()
        indptr, items, order = np.asarray(x.indptr, np.int64), np.ascontiguousarray(x.indices, np.int32), None
        row = np.repeat(np.arange(len(rows), dtype=np.int64), np.diff(indptr))
    if items.size > 1 and np.any((items[1:] == items[:-1]) & (row[1:] == row[:-1])):
        raise ValueError("a target row repeats an item")
    return np.ascontiguousarray(indptr, np.int64), items, order


def rank_call(fn, rows, targets, exclude):
    """Shared body of ``SvdModel.rank_items`` / ``FmModel.rank_items``: fn(indptr, items, x_indptr, x_items, out) -> rc."""
    indptr, items, order = target_csr(targets, rows)
    xp, xi = exclusion_csr(exclude, rows)
    out = np.empty(items.size, np.int32)
    fn(L.ptr_i64(indptr), L.ptr_i32(items), None if xp is None else L.ptr_i64(xp), None if xi is None else L.ptr_i32(xi),
       L.ptr_i32(out))
    if order is None:
        return out
    ranks = np.empty_like(out)
    ranks[order] = out
    return ranks


class SvdModel:
    """The five trainables of ops.py:8-12,29-32 (+ optimiser slots) resident in HBM."""

    def __init__(self, user_num, item_num, dim, *, loss="mse", item_abs=False, reg_bias=False,
                 optimizer="adam", adam_mode="tf1", lr=1e-3, reg=0.05, beta1=0.9, beta2=0.999,
                 eps=1e-8, device=0):
        lib = L.load()
        o = L.TfrOpts()
        lib.tfr_default_opts(C.byref(o))
        o.loss = L.LOSS[loss]
        o.item_abs = int(bool(item_abs))
        o.reg_bias = int(bool(reg_bias))
        o.optimizer = L.OPTIMIZER[optimizer]
        o.adam_mode = L.ADAM_MODE[adam_mode]
        o.device = int(device)
        o.lr, o.reg, o.beta1, o.beta2, o.eps = lr, reg, beta1, beta2, eps
        self._h = L._p()
        self._lib = lib
        self.user_num, self.item_num, self.dim = int(user_num), int(item_num), int(dim)
        self.loss, self.optimizer, self.adam_mode = loss, optimizer, adam_mode
        self.item_abs, self.reg_bias = bool(item_abs), bool(reg_bias)
        self.device = int(device)
        L.check(lib.tfr_create(C.byref(self._h), self.user_num, self.item_num, self.dim, C.byref(o)))

    # -- lifetime -----------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if getattr(self, "_warp", None):             # the WARP trainer goes before the model it is bound to
                self._lib.tfr_warp_destroy(self._warp)
                self._warp = None
            self._lib.tfr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- variables ----------------------------------------------------------------
    def _count(self, which):
        t = which & 7
        return {L.MU: 1, L.BU: self.user_num, L.BI: self.item_num,
                L.P: self.user_num * self.dim, L.Q: self.item_num * self.dim}[t]

    def _shape(self, which):
        t = which & 7
        return {L.MU: (), L.BU: (self.user_num,), L.BI: (self.item_num,),
                L.P: (self.user_num, self.dim), L.Q: (self.item_num, self.dim)}[t]

    def set_table(self, which, values):
        a = L.as_f32(values).reshape(-1)
        L.check(self._lib.tfr_set_table(self._h, which, L.ptr_f32(a), a.size))

    def get_table(self, which):
        out = np.empty(self._count(which), np.float32)
        L.check(self._lib.tfr_get_table(self._h, which, L.ptr_f32(out), out.size))
        return out.reshape(self._shape(which))

    def init_tables(self, seed=0, feature_stddev=0.02, bias_stddev=1.0):
        """tf.global_variables_initializer() (svd_train_val.py:53,56) with the initialisers of
        ops.py:9-12,29-32, drawn on the device."""
        L.check(self._lib.tfr_init_tables(self._h, int(seed), feature_stddev, bias_stddev))

    def set_tables(self, mu, bu, bi, P, Q):
        for which, val in ((L.MU, mu), (L.BU, bu), (L.BI, bi), (L.P, P), (L.Q, Q)):
            self.set_table(which, val)

    def tables(self):
        return {w: self.get_table(w) for w in (L.MU, L.BU, L.BI, L.P, L.Q)}

    def set_frozen(self, mask):
        L.check(self._lib.tfr_set_frozen(self._h, int(mask)))

    def set_hyper(self, lr, reg):
        L.check(self._lib.tfr_set_hyper(self._h, lr, reg))

    @property
    def step(self):
        return self.get_step()[0]

    def get_step(self):
        s, a, b = C.c_int64(), C.c_float(), C.c_float()
        L.check(self._lib.tfr_get_step(self._h, C.byref(s), C.byref(a), C.byref(b)))
        return s.value, a.value, b.value

    def set_step(self, step, beta1_power, beta2_power):
        L.check(self._lib.tfr_set_step(self._h, int(step), beta1_power, beta2_power))

    # -- forward / train ----------------------------------------------------------
    def forward(self, users, items):
        u, i = L.as_i32(users, "user ids"), L.as_i32(items, "item ids")
        if u.shape != i.shape or u.ndim != 1:
            raise ValueError("user and item batches must be 1-D and of equal length")
        out = np.empty(u.size, np.float32)
        L.check(self._lib.tfr_forward(self._h, L.ptr_i32(u), L.ptr_i32(i), u.size, L.ptr_f32(out)))
        return out

    def eval(self, users, items, rates):
        u, i, r = L.as_i32(users, "user ids"), L.as_i32(items, "item ids"), L.as_f32(rates)
        if not (u.shape == i.shape == r.shape) or u.ndim != 1:
            raise ValueError("batches must be 1-D and of equal length")
        sse, neq = C.c_double(), C.c_int64()
        L.check(self._lib.tfr_eval(self._h, L.ptr_i32(u), L.ptr_i32(i), L.ptr_f32(r), u.size,
                                   C.byref(sse), C.byref(neq)))
        return sse.value, neq.value

    # -- bf16 snapshot: predict and evaluate at half the row bytes (bf16.py) ----
    def snapshot_bf16(self):
        """Build or refresh the bf16 copy of the tables the ``*_bf16`` calls score from; training does not move it."""
        L.check(self._lib.tfr_bf16_snapshot(self._h))

    def drop_bf16(self):
        L.check(self._lib.tfr_bf16_drop(self._h))

    def forward_bf16(self, users, items):
        u, i = L.as_i32(users, "user ids"), L.as_i32(items, "item ids")
        if u.shape != i.shape or u.ndim != 1:
            raise ValueError("user and item batches must be 1-D and of equal length")
        out = np.empty(u.size, np.float32)
        L.check(self._lib.tfr_bf16_forward(self._h, L.ptr_i32(u), L.ptr_i32(i), u.size, L.ptr_f32(out)))
        return out

    def forward_bf16_dev(self, d_user, d_item, batch, d_logits):
        L.check(self._lib.tfr_bf16_forward_dev(self._h, d_user, d_item, int(batch), d_logits))

    def eval_bf16(self, users, items, rates):
        """(sse, n_equal) from the snapshot, or (sse, n_equal, nll_sum) under the NLL head."""
        u, i, r = L.as_i32(users, "user ids"), L.as_i32(items, "item ids"), L.as_f32(rates)
        if not (u.shape == i.shape == r.shape) or u.ndim != 1:
            raise ValueError("batches must be 1-D and of equal length")
        sse, neq, nll = C.c_double(), C.c_int64(), C.c_double()
        L.check(self._lib.tfr_bf16_eval(self._h, L.ptr_i32(u), L.ptr_i32(i), L.ptr_f32(r), u.size,
                                        C.byref(sse), C.byref(neq), C.byref(nll)))
        return (sse.value, neq.value, nll.value) if self.loss == "nll" else (sse.value, neq.value)

    def bf16_rows(self, which):
        """The snapshot's rows of ``which`` (P or Q) as the library stores them: uint16 [rows, DP]."""
        rows = self.user_num if which == L.P else self.item_num
        out = np.empty((rows, self._lib.tfr_bf16_row_stride(self.dim)), np.uint16)
        L.check(self._lib.tfr_bf16_get_rows(self._h, int(which), out.ctypes.data_as(C.POINTER(C.c_uint16)), out.size))
        return out

    def upload_eval_triples(self, users, items, rates):
        u, i, r = L.as_i32(users, "user ids"), L.as_i32(items, "item ids"), L.as_f32(rates)
        L.check(self._lib.tfr_upload_eval_triples(self._h, L.ptr_i32(u), L.ptr_i32(i), L.ptr_f32(r), u.size))

    def eval_resident(self):
        """(sum of squared errors, number of infer == rate, n) over the resident validation set."""
        sse, neq, n = C.c_double(), C.c_int64(), C.c_int64()
        L.check(self._lib.tfr_eval_resident(self._h, C.byref(sse), C.byref(neq), C.byref(n)))
        return sse.value, neq.value, n.value

    def eval_binary(self, users, items, rates):
        """The fork's epoch metrics on the device (svd_train_val.py:94-98,170-178): dict(acc, mean_nll, auc, n)."""
        u, i, r = L.as_i32(users, "user ids"), L.as_i32(items, "item ids"), L.as_f32(rates)
        if not (u.shape == i.shape == r.shape) or u.ndim != 1:
            raise ValueError("batches must be 1-D and of equal length")
        neq, nll, auc = C.c_int64(), C.c_double(), C.c_double()
        L.check(self._lib.tfr_eval_binary(self._h, L.ptr_i32(u), L.ptr_i32(i), L.ptr_f32(r), u.size,
                                          C.byref(neq), C.byref(nll), C.byref(auc)))
        n = max(1, u.size)
        return dict(acc=neq.value / n, mean_nll=nll.value / n, auc=auc.value, n=u.size)

    def eval_binary_resident(self):
        neq, nll, auc, n = C.c_int64(), C.c_double(), C.c_double(), C.c_int64()
        L.check(self._lib.tfr_eval_binary_resident(self._h, C.byref(neq), C.byref(nll), C.byref(auc), C.byref(n)))
        return dict(acc=neq.value / max(1, n.value), mean_nll=nll.value / max(1, n.value), auc=auc.value, n=n.value)

    def last_batch_auc(self):
        """AUC of the batch the last ``train_step`` / ``train_steps_repeat`` (with logits) ran on - svd_train_val.py:97 on
        the device: that batch's rates against the logits the call returned.  The batch stays in the handle's workspace, so
        ask right after the step: any other training call, ``forward``, ``forward_resident``, ``eval``, ``eval_binary*``,
        ``forward_bf16`` / ``eval_bf16`` or a call that makes the workspace grow forgets it, and this then raises
        ``TfrError`` (``ERR_STATE``) rather than rank other numbers (include/tfrecomm.h tfr_last_batch_auc)."""
        auc = C.c_double()
        L.check(self._lib.tfr_last_batch_auc(self._h, C.byref(auc)))
        return auc.value

    def auc_dev(self, d_score, d_label, n):
        auc = C.c_double()
        L.check(self._lib.tfr_auc_dev(self._h, d_score, d_label, int(n), C.byref(auc)))
        return auc.value

    def train_step(self, users, items, rates, want_logits=True):
        u, i, r = L.as_i32(users, "user ids"), L.as_i32(items, "item ids"), L.as_f32(rates)
        if not (u.shape == i.shape == r.shape) or u.ndim != 1:
            raise ValueError("batches must be 1-D and of equal length")
        logits = np.empty(u.size, np.float32) if want_logits else None
        loss, reg = C.c_float(), C.c_float()
        L.check(self._lib.tfr_train_step(self._h, L.ptr_i32(u), L.ptr_i32(i), L.ptr_f32(r), u.size,
                                         L.ptr_f32(logits) if want_logits else None,
                                         C.byref(loss), C.byref(reg)))
        return logits, loss.value, reg.value

    def train_steps_repeat(self, users, items, rates, nsteps, want_logits=True, want_loss=True):
        """``for _ in range(nsteps): sess.run(train_op, feed_dict)`` on ONE batch (the per-user fine-tuning loops of
        adaptive_test.py:104-116 / non_adaptive_test.py:82-87) without a host round trip between the steps.
        Returns (pre-update logits of the last step, data loss per step)."""
        u, i, r = L.as_i32(users, "user ids"), L.as_i32(items, "item ids"), L.as_f32(rates)
        if not (u.shape == i.shape == r.shape) or u.ndim != 1:
            raise ValueError("batches must be 1-D and of equal length")
        logits = np.empty(u.size, np.float32) if want_logits else None
        loss = np.empty(int(nsteps), np.float32) if want_loss else None
        L.check(self._lib.tfr_train_steps_repeat(self._h, L.ptr_i32(u), L.ptr_i32(i), L.ptr_f32(r), u.size, int(nsteps),
                                                 L.ptr_f32(logits) if want_logits else None,
                                                 L.ptr_f32(loss) if want_loss else None))
        return logits, loss

    # -- batched per-user fine-tuning (include/tfrecomm.h tfr_finetune_users) --------------------------
    def finetune_users(self, users, row_ptr, items, rates, round_ptr, ask_items, prefix_len, nsteps, round_seq=None,
                       want_loss=True, want_final=True):
        """Every user's rounds of a fine-tuning schedule in one launch (``finetune.adaptive_schedule`` /
        ``finetune.non_adaptive_schedule`` build one).
        User ``users[x]`` trains on rows ``[row_ptr[x], row_ptr[x+1])`` of ``items`` / ``rates``; its rounds are
        ``[round_ptr[x], round_ptr[x+1])``: round ``k`` predicts ``ask_items[k]``, then runs ``nsteps`` steps on the user's
        first ``prefix_len[k]`` rows.  ``round_seq[k]``: the step (from this call's start) at which the sequential drivers
        would start round ``k`` (None = ``k * nsteps``).  Needs mu and the item tables frozen and SGD or lazy Adam.
        Returns (ask logits [n_rounds], data loss of each round's last step [n_rounds] or None, pre-update logits of
        each user's last step over its last round's prefix [n_rows] or None; NaN at rows past that prefix)."""
        u = L.as_i32(users, "user ids").reshape(-1)
        rp = np.ascontiguousarray(np.asarray(row_ptr, np.int64)).reshape(-1)
        it = L.as_i32(items, "item ids").reshape(-1)
        r = L.as_f32(rates).reshape(-1)
        kp = np.ascontiguousarray(np.asarray(round_ptr, np.int64)).reshape(-1)
        ask = L.as_i32(ask_items, "asked item ids").reshape(-1)
        pre = L.as_i32(prefix_len, "prefix lengths").reshape(-1)
        if rp.size != u.size + 1 or kp.size != u.size + 1:
            raise ValueError("row_ptr and round_ptr must hold n_users + 1 offsets")
        n_rows, n_rounds = int(rp[-1]), int(kp[-1])
        if it.size != n_rows or r.size != n_rows:
            raise ValueError("items and rates must hold row_ptr[-1] = %d entries" % n_rows)
        if ask.size != n_rounds or pre.size != n_rounds:
            raise ValueError("ask_items and prefix_len must hold round_ptr[-1] = %d entries" % n_rounds)
        seq = None
        if round_seq is not None:
            seq = np.ascontiguousarray(np.asarray(round_seq, np.int64)).reshape(-1)
            if seq.size != n_rounds:
                raise ValueError("round_seq must hold one position per round")
        ask_out = np.empty(n_rounds, np.float32)
        loss = np.empty(n_rounds, np.float32) if want_loss else None
        final = np.full(n_rows, np.nan, np.float32) if want_final else None
        L.check(self._lib.tfr_finetune_users(self._h, u.size, L.ptr_i32(u), L.ptr_i64(rp), L.ptr_i32(it), L.ptr_f32(r),
                                             L.ptr_i64(kp), L.ptr_i32(ask), L.ptr_i32(pre),
                                             None if seq is None else L.ptr_i64(seq), int(nsteps), L.ptr_f32(ask_out),
                                             None if loss is None else L.ptr_f32(loss),
                                             None if final is None else L.ptr_f32(final)))
        return ask_out, loss, final

    # -- top-K recommendation (forward.py:47-61 get_ranking; include/tfrecomm.h tfr_topk) ---------------
    def recommend(self, users, k=10, exclude=None, return_scores=True):
        """The ``k`` best items for each of ``users`` by score ``((P[u].Q'[i] + mu) + bu[u]) + bi[i]`` (the logit under the
        NLL head), best first, equal scores by item id.  ``exclude``: None, an (indptr, indices) CSR aligned with ``users``,
        or a ``scipy.sparse`` ``[user_num, item_num]`` matrix of rated items (``rated_matrix``).  Returns ``items`` int32
        ``[n, k]`` (-1 past the eligible items) and, if asked, ``scores`` float32 ``[n, k]`` (-inf there)."""
        return self._recommend(self._lib.tfr_topk, users, k, exclude, return_scores)

    def recommend_dev(self, users, k=10, exclude=None, return_scores=True):
        """``recommend`` on torch device tensors (``users`` int32; ``exclude`` None or an (indptr int64, items int32) pair
        of device tensors aligned with ``users``), asynchronous: ordered after torch's current stream, and that stream
        after it.  An id or order error in the inputs surfaces at the next ``sync()``."""
        return self._recommend_dev(self._lib.tfr_topk_dev, users, k, exclude, return_scores)

    def recommend_bf16(self, users, k=10, exclude=None, return_scores=True):
        """``recommend`` from the bf16 snapshot (``snapshot_bf16``): the same arguments and return values, the scores of the
        snapshot's tables with the dot taken 16 features per bf16 matrix instruction (include/tfrecomm.h tfr_bf16_topk)."""
        return self._recommend(self._lib.tfr_bf16_topk, users, k, exclude, return_scores)

    def recommend_bf16_dev(self, users, k=10, exclude=None, return_scores=True):
        """``recommend_dev`` from the bf16 snapshot: the same arguments, return values and stream ordering."""
        return self._recommend_dev(self._lib.tfr_bf16_topk_dev, users, k, exclude, return_scores)

    def _recommend(self, entry, users, k, exclude, return_scores):
        u = L.as_i32(users, "user ids").reshape(-1)
        indptr, excl = exclusion_csr(exclude, u)
        items = np.empty((u.size, int(k)), np.int32)
        scores = np.empty((u.size, int(k)), np.float32) if return_scores else None
        L.check(entry(self._h, L.ptr_i32(u), u.size, int(k),
                      None if indptr is None else L.ptr_i64(indptr), None if excl is None else L.ptr_i32(excl),
                      L.ptr_i32(items), None if scores is None else L.ptr_f32(scores)))
        return (items, scores) if return_scores else items

    def _recommend_dev(self, entry, users, k, exclude, return_scores):
        import torch
        users = users.contiguous()
        if users.dtype != torch.int32 or users.dim() != 1:
            raise TypeError("users must be a 1-D int32 tensor")
        n, k = users.numel(), int(k)
        items = torch.empty((n, k), dtype=torch.int32, device=users.device)
        scores = torch.empty((n, k), dtype=torch.float32, device=users.device) if return_scores else None
        ip = ex = None
        if exclude is not None:
            ip, ex = exclude[0].contiguous(), exclude[1].contiguous()
            if ip.dtype != torch.int64 or ex.dtype != torch.int32 or ip.numel() != n + 1:
                raise TypeError("exclude must be (indptr int64 [n+1], items int32) device tensors")
        mine = torch.cuda.ExternalStream(self.get_stream(), device=users.device)
        cur = torch.cuda.current_stream(users.device)
        mine.wait_stream(cur)
        L.check(entry(self._h, users.data_ptr(), n, k, None if ip is None else ip.data_ptr(),
                      None if ex is None else ex.data_ptr(), items.data_ptr(),
                      None if scores is None else scores.data_ptr()))
        cur.wait_stream(mine)                          # (so no record_stream: the tensors' next users on `cur` come after)
        return (items, scores) if return_scores else items

    # -- nearest neighbours in factor space (include/tfrecomm.h tfr_neighbours) --------------------
    def _similar(self, which, n_rows, rows, k, metric, exclude, lo, hi, return_scores, entry=None):
        from . import neighbours as nb
        entry = entry or self._lib.tfr_neighbours

        def call(*args):
            L.check(entry(self._h, which, *args))
        return nb.query_host(call, rows, n_rows, k, metric, exclude, lo, hi, return_scores)

    def _similar_dev(self, which, n_rows, rows, k, metric, exclude, lo, hi, return_scores, entry=None):
        import torch
        from . import neighbours as nb
        entry = entry or self._lib.tfr_neighbours_dev

        def call(device, *args):
            mine = torch.cuda.ExternalStream(self.get_stream(), device=device)
            cur = torch.cuda.current_stream(device)
            mine.wait_stream(cur)
            L.check(entry(self._h, which, *args))
            cur.wait_stream(mine)
        return nb.query_dev(call, rows, n_rows, k, metric, exclude, lo, hi, return_scores)

    def similar_items(self, items, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """The ``k`` items most like each of ``items`` in factor space, best first, equal scores by item id; an item is never
        its own neighbour.  ``metric``: ``"cosine"`` (``(Q'[a].Q'[b] / |Q'[a]|) / |Q'[b]|``, a zero row scores 0 against
        everything) or ``"dot"`` (``Q'[a].Q'[b]``); ``Q' = |Q|`` under ``item_abs``.  ``exclude``: None, an (indptr, ids) CSR
        aligned with ``items`` or a ``scipy.sparse`` ``[item_num, item_num]`` matrix of items never to return;
        ``lo`` / ``hi`` restrict the candidates to items ``[lo, hi)``.  Returns ``ids`` int32 ``[n, k]`` (-1 past the
        eligible items) and, if asked, ``scores`` float32 ``[n, k]`` (-inf there)."""
        return self._similar(L.NB_ITEMS, self.item_num, items, k, metric, exclude, lo, hi, return_scores)

    def similar_users(self, users, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """``similar_items`` over the rows of ``P``: the ``k`` users most like each of ``users``."""
        return self._similar(L.NB_USERS, self.user_num, users, k, metric, exclude, lo, hi, return_scores)

    def similar_items_dev(self, items, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """``similar_items`` on torch device tensors (``items`` int32; ``exclude`` None or an (indptr int64, ids int32) pair
        aligned with ``items``), asynchronous as ``recommend_dev``: an id or order error surfaces at the next ``sync()``."""
        return self._similar_dev(L.NB_ITEMS, self.item_num, items, k, metric, exclude, lo, hi, return_scores)

    def similar_users_dev(self, users, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """``similar_users`` on torch device tensors, asynchronous as ``recommend_dev``."""
        return self._similar_dev(L.NB_USERS, self.user_num, users, k, metric, exclude, lo, hi, return_scores)

    def similar_items_bf16(self, items, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """``similar_items`` from the bf16 snapshot (``snapshot_bf16``): the same arguments and return values, on the rows of
        the snapshot's ``Q`` with the dot taken 16 features per bf16 matrix instruction and the norms of the snapshot's
        values (include/tfrecomm.h tfr_bf16_neighbours).  The float32 tables are not read."""
        return self._similar(L.NB_ITEMS, self.item_num, items, k, metric, exclude, lo, hi, return_scores,
                             self._lib.tfr_bf16_neighbours)

    def similar_users_bf16(self, users, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """``similar_users`` from the bf16 snapshot: ``similar_items_bf16`` over the rows of the snapshot's ``P``."""
        return self._similar(L.NB_USERS, self.user_num, users, k, metric, exclude, lo, hi, return_scores,
                             self._lib.tfr_bf16_neighbours)

    def similar_items_bf16_dev(self, items, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """``similar_items_dev`` from the bf16 snapshot: the same arguments, return values and stream ordering."""
        return self._similar_dev(L.NB_ITEMS, self.item_num, items, k, metric, exclude, lo, hi, return_scores,
                                 self._lib.tfr_bf16_neighbours_dev)

    def similar_users_bf16_dev(self, users, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """``similar_users_dev`` from the bf16 snapshot: the same arguments, return values and stream ordering."""
        return self._similar_dev(L.NB_USERS, self.user_num, users, k, metric, exclude, lo, hi, return_scores,
                                 self._lib.tfr_bf16_neighbours_dev)

    # -- held-out ranking (include/tfrecomm.h tfr_rank_items; tfrecomm_amd.ranking for the metrics) -------------
    def rank_items(self, users, targets, exclude=None):
        """0-based rank of each target item of each of ``users`` among all items not in ``exclude``: the number of eligible
        items with a non-NaN score whose key (score descending, then item id ascending, as ``recommend``) beats the target's.
        -1 for a target that is excluded or scores NaN.  ``rank < k`` exactly when the target is in ``recommend(users, k,
        exclude)``, at that position.  ``targets``: an (indptr, items) pair aligned with ``users`` (ranks aligned with those
        items) or a ``scipy.sparse`` ``[user_num, item_num]`` matrix (ranks aligned with its rows for ``users``, indices
        sorted); ``exclude`` as in ``recommend``.  Returns int32 ranks."""
        u = L.as_i32(users, "user ids").reshape(-1)

        def call(ip, it, xp, xi, out):
            L.check(self._lib.tfr_rank_items(self._h, L.ptr_i32(u), u.size, ip, it, xp, xi, out))
        return rank_call(call, u, targets, exclude)

    def rank_items_bf16(self, users, targets, exclude=None):
        """``rank_items`` from the bf16 snapshot (``snapshot_bf16``): the same arguments and return values, by the keys of
        ``recommend_bf16``, so ``rank < k`` exactly when the target is in ``recommend_bf16(users, k, exclude)``, at that
        position (include/tfrecomm.h tfr_bf16_rank_items).  The float32 tables are not read."""
        u = L.as_i32(users, "user ids").reshape(-1)

        def call(ip, it, xp, xi, out):
            L.check(self._lib.tfr_bf16_rank_items(self._h, L.ptr_i32(u), u.size, ip, it, xp, xi, out))
        return rank_call(call, u, targets, exclude)

    # -- resident store -----------------------------------------------------------
    def upload_triples(self, users, items, rates):
        u, i, r = L.as_i32(users, "user ids"), L.as_i32(items, "item ids"), L.as_f32(rates)
        L.check(self._lib.tfr_upload_triples(self._h, L.ptr_i32(u), L.ptr_i32(i), L.ptr_f32(r), u.size))

    def set_triples_dev(self, d_user, d_item, d_rate, n):
        L.check(self._lib.tfr_set_triples_dev(self._h, d_user, d_item, d_rate, n))

    def train_steps_resident(self, ids, batch, want_loss=True):
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64)).reshape(-1)
        if ids.size % batch:
            raise ValueError("ids length must be a multiple of batch")
        n = ids.size // batch
        loss = np.empty(n, np.float32) if want_loss else None
        L.check(self._lib.tfr_train_steps_resident(self._h, L.ptr_i64(ids), batch, n,
                                                   L.ptr_f32(loss) if want_loss else None))
        return loss

    def stage_ids(self, ids):
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64)).reshape(-1)
        L.check(self._lib.tfr_stage_ids(self._h, L.ptr_i64(ids), ids.size))

    def train_steps_staged(self, first_step, batch, nsteps, want_loss=False):
        loss = np.empty(nsteps, np.float32) if want_loss else None
        L.check(self._lib.tfr_train_steps_staged(self._h, first_step, batch, nsteps,
                                                 L.ptr_f32(loss) if want_loss else None))
        return loss

    # -- the ShuffleIterator id draw on the device (dataio.py:115; include/tfrecomm.h "id draw") -----
    def rng_seed(self, seed):
        """``np.random.seed(seed)`` for the device generator (svd_train_val.py:15)."""
        L.check(self._lib.tfr_rng_seed(self._h, int(seed) & 0xFFFFFFFF))

    def rng_set_state(self, key, pos):
        k = np.ascontiguousarray(np.asarray(key, dtype=np.uint32)).reshape(-1)
        if k.size != 624:
            raise ValueError("MT19937 key must hold 624 words")
        L.check(self._lib.tfr_rng_set_state(self._h, k.ctypes.data_as(C.POINTER(C.c_uint32)), int(pos)))

    def rng_get_state(self):
        k, pos = np.empty(624, np.uint32), C.c_int32()
        L.check(self._lib.tfr_rng_get_state(self._h, k.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(pos)))
        return k, pos.value

    def rng_from_numpy(self):
        """Hand NumPy's legacy global generator (the one dataio.ShuffleIterator draws from) to the device."""
        st = np.random.get_state()
        if st[0] != "MT19937":
            raise RuntimeError("NumPy's legacy generator is not MT19937")
        self.rng_set_state(st[1], st[2])

    def rng_to_numpy(self):
        """...and back: host draws after this continue the stream where the device left it."""
        k, pos = self.rng_get_state()
        st = np.random.get_state()
        np.random.set_state((st[0], k, pos, st[3], st[4]))

    def draw_ids(self, high, count):
        """``np.random.randint(0, high, (count,))`` drawn on the device (int64, bit-identical stream)."""
        out = np.empty(int(count), np.int64)
        L.check(self._lib.tfr_draw_ids(self._h, int(high), out.size, L.ptr_i64(out)))
        return out

    def draw_ids_dev(self, high, count, d_out):
        """``np.random.randint(0, high, (count,))`` into device memory (pointer), asynchronously on the draw stream"""
        L.check(self._lib.tfr_draw_ids_dev(self._h, int(high), int(count), d_out))

    def join_draws(self):
        """the model's stream waits for every draw issued by ``draw_ids_dev`` so far"""
        L.check(self._lib.tfr_join_draws(self._h))

    def join_draw(self, ordinal):
        """...for the first ``ordinal`` draws issued (counted from 1) only"""
        L.check(self._lib.tfr_join_draw(self._h, int(ordinal)))

    def train_steps_drawn(self, batch, nsteps, want_loss=False):
        """nsteps x { next(iter_train); sess.run(train_op) } with the id draw, the gather from the resident
        store and the step all on the device."""
        loss = np.empty(nsteps, np.float32) if want_loss else None
        L.check(self._lib.tfr_train_steps_drawn(self._h, int(batch), int(nsteps), L.ptr_f32(loss) if want_loss else None))
        return loss

    def train_step_ids(self, ids):
        """One step on store rows ``ids`` (host int64, e.g. straight from np.random.randint); asynchronous."""
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int64)).reshape(-1)
        L.check(self._lib.tfr_train_step_ids(self._h, L.ptr_i64(a), a.size))

    def forward_resident(self, lo, hi):
        out = np.empty(hi - lo, np.float32)
        L.check(self._lib.tfr_forward_resident(self._h, lo, hi, L.ptr_f32(out)))
        return out

    def sort_segments(self, side, ids):
        a = L.as_i32(ids)
        ks, ps = np.empty(a.size, np.int32), np.empty(a.size, np.int32)
        L.check(self._lib.tfr_sort_segments(self._h, side, L.ptr_i32(a), a.size, L.ptr_i32(ks), L.ptr_i32(ps)))
        return ks, ps

    # -- BPR on implicit feedback (include/tfrecomm.h tfr_bpr_*) ------------------------------------------
    def set_positives(self, csr):
        """The positives of the BPR steps: a ``scipy.sparse`` ``[user_num, item_num]`` matrix (e.g. ``rated_matrix``; its
        stored entries) or an (indptr, items) pair with strictly increasing rows.  Checked before any device work."""
        from .svdpp import implicit_csr
        indptr, items = implicit_csr(csr, self.user_num, self.item_num)
        L.check(self._lib.tfr_bpr_set_positives(self._h, L.ptr_i64(indptr), L.ptr_i32(items)))

    def set_bpr_sampler(self, seed=0, attempts=16):
        L.check(self._lib.tfr_bpr_set_sampler(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(attempts)))

    def bpr_negatives(self, users, step=None):
        """The sampler alone for ``users`` at counter ``step`` (default: the model's step counter, i.e. what the next
        step would draw).  int32 negatives, -1 where every attempt landed on a positive."""
        u = L.as_i32(users, "user ids").reshape(-1)
        out = np.empty(u.size, np.int32)
        L.check(self._lib.tfr_bpr_negatives(self._h, L.ptr_i32(u), u.size, self.step if step is None else int(step),
                                            L.ptr_i32(out)))
        return out

    def train_bpr_step(self, users, pos_items, neg_items=None):
        """One BPR step on host columns; ``neg_items`` None = sample on the device.  Returns (negatives used, data loss,
        regulariser, number of skipped triples)."""
        u, i = L.as_i32(users, "user ids").reshape(-1), L.as_i32(pos_items, "item ids").reshape(-1)
        j = None if neg_items is None else L.as_i32(neg_items, "item ids").reshape(-1)
        if u.shape != i.shape or (j is not None and j.shape != u.shape):
            raise ValueError("batches must be 1-D and of equal length")
        neg = np.empty(u.size, np.int32)
        loss, reg, skipped = C.c_float(), C.c_float(), C.c_int64()
        L.check(self._lib.tfr_bpr_train_step(self._h, L.ptr_i32(u), L.ptr_i32(i), None if j is None else L.ptr_i32(j),
                                             u.size, L.ptr_i32(neg), C.byref(loss), C.byref(reg), C.byref(skipped)))
        return neg, loss.value, reg.value, skipped.value

    def train_bpr_step_dev(self, users, pos_items, neg_items=None, want_negatives=False):
        """One BPR step on torch int32 device tensors, asynchronous: ordered after torch's current stream, and that stream
        after it; an id error surfaces at the next ``sync()``.  Returns the negatives as a device tensor when asked."""
        import torch
        cols = [users.contiguous(), pos_items.contiguous()] + ([] if neg_items is None else [neg_items.contiguous()])
        if any(c.dtype != torch.int32 or c.dim() != 1 or c.shape != cols[0].shape for c in cols):
            raise TypeError("users / items must be 1-D int32 tensors of equal length")
        n = cols[0].numel()
        neg = torch.empty(n, dtype=torch.int32, device=cols[0].device) if want_negatives else None
        mine = torch.cuda.ExternalStream(self.get_stream(), device=cols[0].device)
        cur = torch.cuda.current_stream(cols[0].device)
        mine.wait_stream(cur)
        L.check(self._lib.tfr_bpr_train_step_dev(self._h, cols[0].data_ptr(), cols[1].data_ptr(),
                                                 None if neg_items is None else cols[2].data_ptr(), n,
                                                 None if neg is None else neg.data_ptr()))
        cur.wait_stream(mine)
        return neg

    def train_bpr_steps_drawn(self, batch, nsteps, want_loss=False):
        """nsteps x { e = np.random.randint(0, nnz, batch) (the device generator, as ``train_steps_drawn``); (u, i) =
        entry e of the positives; one BPR step with sampled negatives }, all on the device.  Per-step data loss if asked."""
        loss = np.empty(nsteps, np.float32) if want_loss else None
        L.check(self._lib.tfr_bpr_train_steps_drawn(self._h, int(batch), int(nsteps),
                                                    L.ptr_f32(loss) if want_loss else None))
        return loss

    # -- WARP on implicit feedback (include/tfrecomm.h tfr_warp_*) ----------------------------------------
    def set_warp(self, margin=1.0):
        """The margin of the WARP steps.  The trainer handle is created by the first call and closed before the model; the
        positives and the sampler's seed and attempts are the BPR ones (``set_positives``, ``set_bpr_sampler``)."""
        if getattr(self, "_warp", None):
            L.check(self._lib.tfr_warp_set_margin(self._warp, float(margin)))
            return
        h = L._p()
        L.check(self._lib.tfr_warp_create(C.byref(h), self._h, float(margin)))
        self._warp = h

    def _warp_handle(self):
        if not getattr(self, "_warp", None):
            self.set_warp()
        return self._warp

    def warp_negatives(self, users, pos_items, step=None):
        """The violator search alone on the current tables, at counter ``step`` (default: the model's step counter, i.e.
        what the next step would find).  Returns (int32 negatives, -1 where no candidate violates the margin; int32 trial
        counts N, 0 there)."""
        u, i = L.as_i32(users, "user ids").reshape(-1), L.as_i32(pos_items, "item ids").reshape(-1)
        if u.shape != i.shape:
            raise ValueError("batches must be 1-D and of equal length")
        neg, trials = np.empty(u.size, np.int32), np.empty(u.size, np.int32)
        L.check(self._lib.tfr_warp_negatives(self._warp_handle(), L.ptr_i32(u), L.ptr_i32(i), u.size,
                                             self.step if step is None else int(step), L.ptr_i32(neg), L.ptr_i32(trials)))
        return neg, trials

    def train_warp_step(self, users, pos_items, neg_items=None):
        """One WARP step on host columns; ``neg_items`` None = search on the device.  Returns (negatives used, trial counts,
        data loss, regulariser, number of skipped triples)."""
        u, i = L.as_i32(users, "user ids").reshape(-1), L.as_i32(pos_items, "item ids").reshape(-1)
        j = None if neg_items is None else L.as_i32(neg_items, "item ids").reshape(-1)
        if u.shape != i.shape or (j is not None and j.shape != u.shape):
            raise ValueError("batches must be 1-D and of equal length")
        neg, trials = np.empty(u.size, np.int32), np.empty(u.size, np.int32)
        loss, reg, skipped = C.c_float(), C.c_float(), C.c_int64()
        L.check(self._lib.tfr_warp_train_step(self._warp_handle(), L.ptr_i32(u), L.ptr_i32(i),
                                              None if j is None else L.ptr_i32(j), u.size, L.ptr_i32(neg), L.ptr_i32(trials),
                                              C.byref(loss), C.byref(reg), C.byref(skipped)))
        return neg, trials, loss.value, reg.value, skipped.value

    def train_warp_step_dev(self, users, pos_items, neg_items=None, want_negatives=False):
        """One WARP step on torch int32 device tensors, asynchronous: ordered after torch's current stream, and that stream
        after it; an id error surfaces at the next ``sync()``.  Returns (negatives, trial counts) as device tensors when
        asked."""
        import torch
        cols = [users.contiguous(), pos_items.contiguous()] + ([] if neg_items is None else [neg_items.contiguous()])
        if any(c.dtype != torch.int32 or c.dim() != 1 or c.shape != cols[0].shape for c in cols):
            raise TypeError("users / items must be 1-D int32 tensors of equal length")
        n = cols[0].numel()
        neg = torch.empty(n, dtype=torch.int32, device=cols[0].device) if want_negatives else None
        trials = torch.empty(n, dtype=torch.int32, device=cols[0].device) if want_negatives else None
        w = self._warp_handle()
        mine = torch.cuda.ExternalStream(self.get_stream(), device=cols[0].device)
        cur = torch.cuda.current_stream(cols[0].device)
        mine.wait_stream(cur)
        L.check(self._lib.tfr_warp_train_step_dev(w, cols[0].data_ptr(), cols[1].data_ptr(),
                                                  None if neg_items is None else cols[2].data_ptr(), n,
                                                  None if neg is None else neg.data_ptr(),
                                                  None if trials is None else trials.data_ptr()))
        cur.wait_stream(mine)
        return (neg, trials) if want_negatives else None

    def train_warp_steps_drawn(self, batch, nsteps, want_loss=False):
        """nsteps x { e = np.random.randint(0, nnz, batch) (the device generator, as ``train_bpr_steps_drawn``); (u, i) =
        entry e of the positives; one WARP step with the search }, all on the device.  Per-step data loss if asked."""
        loss = np.empty(nsteps, np.float32) if want_loss else None
        L.check(self._lib.tfr_warp_train_steps_drawn(self._warp_handle(), int(batch), int(nsteps),
                                                     L.ptr_f32(loss) if want_loss else None))
        return loss

    # -- device-pointer plumbing --------------------------------------------------
    def forward_dev(self, d_user, d_item, batch, d_logits):
        L.check(self._lib.tfr_forward_dev(self._h, d_user, d_item, batch, d_logits))

    def train_step_dev(self, d_user, d_item, d_rate, batch, d_logits=None):
        L.check(self._lib.tfr_train_step_dev(self._h, d_user, d_item, d_rate, batch, d_logits))

    # -- row-sharded building blocks (device pointers; see include/tfrecomm.h) ------
    def shard_row_stride(self):
        return int(self._lib.tfr_shard_row_stride(self._h))

    def shard_route(self, d_user, d_item, d_rate, batch_global, rank, world, user_num_global, item_num_global,
                    sample_cap, slot_cap, d_req):
        L.check(self._lib.tfr_shard_route(self._h, d_user, d_item, d_rate, batch_global, rank, world, user_num_global,
                                          item_num_global, sample_cap, slot_cap, d_req))

    def shard_route_ids(self, d_ids, batch_global, rank, world, user_num_global, item_num_global, sample_cap, slot_cap, d_req):
        L.check(self._lib.tfr_shard_route_ids(self._h, d_ids, batch_global, rank, world, user_num_global, item_num_global,
                                              sample_cap, slot_cap, d_req))

    def shard_bucket_ids(self, d_ids, batch, world, user_num_global, pair_cap, d_send):
        L.check(self._lib.tfr_shard_bucket_ids(self._h, d_ids, batch, world, user_num_global, pair_cap, d_send))

    def shard_route_recs(self, d_recs, n, rank, world, user_num_global, item_num_global, sample_cap, slot_cap, d_req):
        L.check(self._lib.tfr_shard_route_recs(self._h, d_recs, n, rank, world, user_num_global, item_num_global,
                                               sample_cap, slot_cap, d_req))

    def shard_routed_devptrs(self):
        ps = [L._p() for _ in range(4)]
        L.check(self._lib.tfr_shard_routed_devptrs(self._h, *[C.byref(p) for p in ps]))
        return tuple(p.value for p in ps)

    def shard_gather(self, d_req_recv, n, d_rows_out):
        L.check(self._lib.tfr_shard_gather(self._h, d_req_recv, n, d_rows_out))

    def shard_forward_reduce(self, d_item_rows, d_logits, d_item_grad, d_scalars4):
        L.check(self._lib.tfr_shard_forward_reduce(self._h, d_item_rows, d_logits, d_item_grad, d_scalars4))

    def shard_forward_items(self, d_item_rows, d_logits, d_item_grad, d_scalars4):
        L.check(self._lib.tfr_shard_forward_items(self._h, d_item_rows, d_logits, d_item_grad, d_scalars4))

    def shard_reduce_users(self, d_item_rows):
        L.check(self._lib.tfr_shard_reduce_users(self._h, d_item_rows))

    def shard_apply_items(self, d_req_recv, d_grad_recv, n):
        L.check(self._lib.tfr_shard_apply_items(self._h, d_req_recv, d_grad_recv, n))

    def shard_select(self, which):
        L.check(self._lib.tfr_shard_select(self._h, int(which)))

    def shard_presort(self, d_req_recv, n):
        L.check(self._lib.tfr_shard_presort(self._h, d_req_recv, int(n)))

    def shard_finish_step(self, d_scalars4):
        L.check(self._lib.tfr_shard_finish_step(self._h, d_scalars4))

    # -- data-parallel building blocks ------------------------------------------------
    def dp_flat_size(self):
        return int(self._lib.tfr_dp_flat_size(self._h))

    def dp_hint_next(self, d_next_store_ids):
        """Look-ahead: the store ids the next ``dp_local_grads`` call will use (device pointer)."""
        L.check(self._lib.tfr_dp_hint_next(self._h, d_next_store_ids))

    def dp_local_grads(self, d_user, d_item, d_rate, batch, d_store_ids, d_flat):
        L.check(self._lib.tfr_dp_local_grads(self._h, d_user, d_item, d_rate, batch, d_store_ids, d_flat))

    def dp_apply(self, d_flat):
        L.check(self._lib.tfr_dp_apply(self._h, d_flat))

    def staged_ids_devptr(self):
        p, n = L._p(), C.c_int64()
        L.check(self._lib.tfr_staged_ids_devptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def table_devptr(self, which):
        p, n = L._p(), C.c_int64()
        L.check(self._lib.tfr_table_devptr(self._h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_stream(self, stream_ptr):
        L.check(self._lib.tfr_set_stream(self._h, stream_ptr))

    def switch_stream(self, stream_ptr):
        """set_stream without draining the stream in use (the caller orders the streams itself)"""
        L.check(self._lib.tfr_switch_stream(self._h, stream_ptr))

    def get_stream(self):
        p = L._p()
        L.check(self._lib.tfr_get_stream(self._h, C.byref(p)))
        return p.value

    def sync(self):
        L.check(self._lib.tfr_sync(self._h))

    # -- per-kernel HIP-event timing ----------------------------------------------
    def profile(self, enable=True):
        L.check(self._lib.tfr_profile(self._h, int(bool(enable))))

    def kernel_plan(self, batch):
        """{slot: kernel symbol} of one training step at this batch size (rocprofv3's spelling)."""
        buf = C.create_string_buffer(1024)
        L.check(self._lib.tfr_kernel_plan(self._h, int(batch), buf, 1024))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";") if kv)

    def profile_read(self):
        out = {}
        for k, name in enumerate(L.KERNEL_NAMES):
            ms, n = C.c_double(), C.c_int64()
            L.check(self._lib.tfr_profile_read(self._h, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out
