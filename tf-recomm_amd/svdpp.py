"""SvdppModel: SVD++ (Koren, "Factorization Meets the Neighborhood", KDD 2008) on the device - the third model the
reference README names.  Thin wrapper over the ``tfr_svdpp`` handle of include/tfrecomm.h.

    z_u   = |N(u)|^-1/2 * sum_{j in N(u)} Y[j]          (0 for an empty N(u))
    logit = ((dot(P[u] + z_u, Q'[i]) + mu) + bu[u]) + bi[i]

N(u), the implicit set of user u, is a fixed CSR [user_num, item_num] given once with ``set_implicit`` (usually the items u
rated in training: ``rated_matrix``).  Holds no arithmetic: every number comes from the HIP kernels.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import exclusion_csr, rank_call

Y = L.Y


def implicit_csr(x, user_num, item_num):
    """N(u) as the C-ABI's (indptr int64 [user_num + 1] from 0, items int32), checked before any device call.

    ``x`` is a ``scipy.sparse`` matrix ``[user_num, item_num]`` (its stored entries; duplicates merged, rows sorted) or an
    (indptr, items) pair whose rows must already be strictly increasing.  A row that is not (unsorted or repeated) or a
    malformed indptr raises ValueError; an item outside [0, item_num) raises OutOfRangeError."""
    user_num, item_num = int(user_num), int(item_num)
    if isinstance(x, tuple):
        indptr, items = x
        indptr = np.asarray(indptr)
        if indptr.dtype.kind not in "iu":
            raise ValueError("implicit indptr must be integer")
        indptr = np.ascontiguousarray(indptr, np.int64).reshape(-1)
        items = L.as_i32(items, "implicit items").reshape(-1)
    else:
        m = x.tocsr(copy=True)
        if m.shape != (user_num, item_num):
            raise ValueError("implicit matrix must be [%d, %d], got %s" % (user_num, item_num, m.shape))
        m.sum_duplicates()                              # also sorts each row
        indptr = np.ascontiguousarray(m.indptr, np.int64)
        items = np.ascontiguousarray(m.indices, np.int32)
    if indptr.size != user_num + 1:
        raise ValueError("implicit indptr must hold user_num + 1 = %d entries, got %d" % (user_num + 1, indptr.size))
    if indptr[0] != 0 or np.any(np.diff(indptr) < 0) or indptr[-1] != items.size:
        raise ValueError("implicit indptr must start at 0, be non-decreasing and end at the number of items")
    if items.size and (items.min() < 0 or items.max() >= item_num):
        raise L.OutOfRangeError(L.ERR_OOB, "implicit item outside [0, %d)" % item_num)
    if items.size > 1:
        row = np.repeat(np.arange(user_num, dtype=np.int64), np.diff(indptr))
        if np.any((items[1:] <= items[:-1]) & (row[1:] == row[:-1])):
            raise ValueError("an implicit row is not strictly increasing (unsorted or repeated items)")
    return indptr, items


class SvdppModel:
    """The five SVD trainables plus Y [item_num, dim] (+ optimiser slots) resident in HBM.  SGD or lazy Adam."""

    def __init__(self, user_num, item_num, dim, *, loss="mse", item_abs=False, reg_bias=False, optimizer="adam",
                 adam_mode="lazy", lr=1e-3, reg=0.05, beta1=0.9, beta2=0.999, eps=1e-8, device=0):
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
        self._check(lib.tfr_svdpp_create(C.byref(self._h), self.user_num, self.item_num, self.dim, C.byref(o)))

    # -- lifetime -----------------------------------------------------------------
    def _check(self, rc):
        if rc != L.OK:
            text = self._lib.tfr_svdpp_last_error().decode("utf-8", "replace")
            raise (L.OutOfRangeError if rc == L.ERR_OOB else L.TfrError)(rc, text)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tfr_svdpp_destroy(self._h)
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
    def _shape(self, which):
        return {L.MU: (), L.BU: (self.user_num,), L.BI: (self.item_num,), L.P: (self.user_num, self.dim),
                L.Q: (self.item_num, self.dim), Y: (self.item_num, self.dim)}[which & 7]

    def set_table(self, which, values):
        a = L.as_f32(values).reshape(-1)
        self._check(self._lib.tfr_svdpp_set_table(self._h, which, L.ptr_f32(a), a.size))

    def get_table(self, which):
        shape = self._shape(which)
        out = np.empty(int(np.prod(shape)), np.float32)
        self._check(self._lib.tfr_svdpp_get_table(self._h, which, L.ptr_f32(out), out.size))
        return out.reshape(shape)

    def set_tables(self, mu, bu, bi, P, Q, Y=None):
        for which, val in ((L.MU, mu), (L.BU, bu), (L.BI, bi), (L.P, P), (L.Q, Q), (L.Y, Y)):
            if val is not None:
                self.set_table(which, val)

    def tables(self):
        """{MU, BU, BI, P, Q, Y}: what a checkpoint of the model holds (``set_tables`` restores it)."""
        return {w: self.get_table(w) for w in (L.MU, L.BU, L.BI, L.P, L.Q, Y)}

    def init_tables(self, seed=0, feature_stddev=0.02, bias_stddev=1.0):
        """The SVD initialisers on the device, and Y ~ truncated normal(feature_stddev); step and slots reset."""
        self._check(self._lib.tfr_svdpp_init(self._h, int(seed), feature_stddev, bias_stddev))

    def set_implicit(self, csr_or_pair):
        """N(u) for every user: a ``scipy.sparse`` [user_num, item_num] (e.g. ``rated_matrix``) or an (indptr, items)
        pair; checked here (``implicit_csr``) before any device call."""
        indptr, items = implicit_csr(csr_or_pair, self.user_num, self.item_num)
        self._check(self._lib.tfr_svdpp_set_implicit(self._h, L.ptr_i64(indptr), L.ptr_i32(items)))

    def set_frozen(self, mask):
        """bit (1 << table) for MU, BU, BI, P, Q and Y = 5: that table receives no update."""
        self._check(self._lib.tfr_svdpp_set_frozen(self._h, int(mask)))

    def set_hyper(self, lr, reg):
        self._check(self._lib.tfr_svdpp_set_hyper(self._h, lr, reg))

    @property
    def step(self):
        return self.get_step()[0]

    def get_step(self):
        s, a, b = C.c_int64(), C.c_float(), C.c_float()
        self._check(self._lib.tfr_svdpp_get_step(self._h, C.byref(s), C.byref(a), C.byref(b)))
        return s.value, a.value, b.value

    def set_step(self, step, beta1_power, beta2_power):
        self._check(self._lib.tfr_svdpp_set_step(self._h, int(step), beta1_power, beta2_power))

    def get_stream(self):
        p = L._p()
        self._check(self._lib.tfr_svdpp_get_stream(self._h, C.byref(p)))
        return p.value

    def sync(self):
        self._check(self._lib.tfr_svdpp_sync(self._h))

    # -- forward / train (host arrays) --------------------------------------------------
    @staticmethod
    def _batch(users, items, rates=None):
        u, i = L.as_i32(users, "user ids"), L.as_i32(items, "item ids")
        r = None if rates is None else L.as_f32(rates)
        if u.shape != i.shape or u.ndim != 1 or (r is not None and r.shape != u.shape):
            raise ValueError("batches must be 1-D and of equal length")
        return u, i, r

    def forward(self, users, items):
        u, i, _ = self._batch(users, items)
        out = np.empty(u.size, np.float32)
        self._check(self._lib.tfr_svdpp_forward(self._h, L.ptr_i32(u), L.ptr_i32(i), u.size, L.ptr_f32(out)))
        return out

    def eval(self, users, items, rates):
        """(sum of squared errors of the head against the rates, number of head == rate)."""
        u, i, r = self._batch(users, items, rates)
        sse, neq = C.c_double(), C.c_int64()
        self._check(self._lib.tfr_svdpp_eval(self._h, L.ptr_i32(u), L.ptr_i32(i), L.ptr_f32(r), u.size, C.byref(sse),
                                             C.byref(neq)))
        return sse.value, neq.value

    def train_step(self, users, items, rates, want_logits=True):
        """One minibatch; returns (pre-update logits or None, data loss, regulariser)."""
        u, i, r = self._batch(users, items, rates)
        logits = np.empty(u.size, np.float32) if want_logits else None
        loss, reg = C.c_float(), C.c_float()
        self._check(self._lib.tfr_svdpp_train_step(self._h, L.ptr_i32(u), L.ptr_i32(i), L.ptr_f32(r), u.size,
                                                   L.ptr_f32(logits) if want_logits else None, C.byref(loss),
                                                   C.byref(reg)))
        return logits, loss.value, reg.value

    # -- torch device tensors: ordered after torch's current stream, and that stream after the call ------------
    def _on_stream(self, device, call):
        import torch
        mine = torch.cuda.ExternalStream(self.get_stream(), device=device)
        cur = torch.cuda.current_stream(device)
        mine.wait_stream(cur)
        call()
        cur.wait_stream(mine)

    @staticmethod
    def _dev_batch(users, items, rates=None):
        import torch
        users, items = users.contiguous(), items.contiguous()
        if users.dtype != torch.int32 or items.dtype != torch.int32 or users.dim() != 1 or users.shape != items.shape:
            raise TypeError("users / items must be 1-D int32 tensors of equal length")
        if rates is not None:
            rates = rates.contiguous()
            if rates.dtype != torch.float32 or rates.shape != users.shape:
                raise TypeError("rates must be a float32 tensor shaped like users")
        return users, items, rates

    def forward_dev(self, users, items):
        """Logits of torch int32 device tensors, as a float32 device tensor (asynchronous)."""
        import torch
        users, items, _ = self._dev_batch(users, items)
        out = torch.empty(users.numel(), dtype=torch.float32, device=users.device)
        if users.numel():
            self._on_stream(users.device, lambda: self._check(self._lib.tfr_svdpp_forward_dev(
                self._h, users.data_ptr(), items.data_ptr(), users.numel(), out.data_ptr())))
        return out

    def train_step_dev(self, users, items, rates, want_logits=False):
        """One minibatch on torch device tensors, asynchronous: an id error surfaces at the next ``sync()``.  Returns the
        pre-update logits as a device tensor when asked, else None."""
        import torch
        users, items, rates = self._dev_batch(users, items, rates)
        logits = torch.empty(users.numel(), dtype=torch.float32, device=users.device) if want_logits else None
        self._on_stream(users.device, lambda: self._check(self._lib.tfr_svdpp_train_step_dev(
            self._h, users.data_ptr(), items.data_ptr(), rates.data_ptr(), users.numel(),
            logits.data_ptr() if logits is not None else None)))
        return logits

    # -- top-K and held-out ranking (the SvdModel signatures; tfrecomm_amd.evaluate_ranking works on this model) ---------
    def recommend(self, users, k=10, exclude=None, return_scores=True):
        """The ``k`` best items per user by ((dot(P[u] + z_u, Q'[i]) + mu) + bu[u]) + bi[i], best first, equal scores by
        item id; ``exclude`` as ``SvdModel.recommend``."""
        u = L.as_i32(users, "user ids").reshape(-1)
        indptr, excl = exclusion_csr(exclude, u)
        items = np.empty((u.size, int(k)), np.int32)
        scores = np.empty((u.size, int(k)), np.float32) if return_scores else None
        self._check(self._lib.tfr_svdpp_topk(self._h, L.ptr_i32(u), u.size, int(k),
                                             None if indptr is None else L.ptr_i64(indptr),
                                             None if excl is None else L.ptr_i32(excl), L.ptr_i32(items),
                                             None if scores is None else L.ptr_f32(scores)))
        return (items, scores) if return_scores else items

    def recommend_dev(self, users, k=10, exclude=None, return_scores=True):
        """``recommend`` on torch device tensors, asynchronous (as ``SvdModel.recommend_dev``)."""
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
        self._on_stream(users.device, lambda: self._check(self._lib.tfr_svdpp_topk_dev(
            self._h, users.data_ptr(), n, k, None if ip is None else ip.data_ptr(), None if ex is None else ex.data_ptr(),
            items.data_ptr(), None if scores is None else scores.data_ptr())))
        return (items, scores) if return_scores else items

    # -- nearest neighbours (the SvdModel signatures; users on the effective rows P[u] + z_u) -------------------------
    def _similar(self, which, n_rows, rows, k, metric, exclude, lo, hi, return_scores):
        from . import neighbours as nb

        def call(*args):
            self._check(self._lib.tfr_svdpp_neighbours(self._h, which, *args))
        return nb.query_host(call, rows, n_rows, k, metric, exclude, lo, hi, return_scores)

    def _similar_dev(self, which, n_rows, rows, k, metric, exclude, lo, hi, return_scores):
        from . import neighbours as nb

        def call(device, *args):
            self._on_stream(device, lambda: self._check(self._lib.tfr_svdpp_neighbours_dev(self._h, which, *args)))
        return nb.query_dev(call, rows, n_rows, k, metric, exclude, lo, hi, return_scores)

    def similar_items(self, items, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """The ``k`` items most like each of ``items`` over the rows of ``Q'``, as ``SvdModel.similar_items``."""
        return self._similar(L.NB_ITEMS, self.item_num, items, k, metric, exclude, lo, hi, return_scores)

    def similar_users(self, users, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """The ``k`` users most like each of ``users`` over the effective rows ``P[u] + z_u`` that ``recommend`` scores with
        (rebuilt for every user by each call; needs the implicit sets)."""
        return self._similar(L.NB_USERS, self.user_num, users, k, metric, exclude, lo, hi, return_scores)

    def similar_items_dev(self, items, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """``similar_items`` on torch device tensors, asynchronous (as ``SvdModel.similar_items_dev``)."""
        return self._similar_dev(L.NB_ITEMS, self.item_num, items, k, metric, exclude, lo, hi, return_scores)

    def similar_users_dev(self, users, k=10, metric="cosine", exclude=None, return_scores=True, lo=0, hi=None):
        """``similar_users`` on torch device tensors, asynchronous."""
        return self._similar_dev(L.NB_USERS, self.user_num, users, k, metric, exclude, lo, hi, return_scores)

    def rank_items(self, users, targets, exclude=None):
        """0-based rank of each target among the eligible items, as ``SvdModel.rank_items``: ``rank < k`` exactly when
        ``recommend(users, k, exclude)`` returns the target, at that position."""
        u = L.as_i32(users, "user ids").reshape(-1)

        def call(ip, it, xp, xi, out):
            self._check(self._lib.tfr_svdpp_rank_items(self._h, L.ptr_i32(u), u.size, ip, it, xp, xi, out))
        return rank_call(call, u, targets, exclude)
