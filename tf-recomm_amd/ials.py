"""``ImplicitALS``: implicit-feedback ALS (Hu, Koren, Volinsky) fitted on the GPU in float64 (csrc/ials.hip).

    m = ImplicitALS(user_num, item_num, factors=32, regularization=0.01, alpha=40.0, iterations=15)
    m.fit(user_items)                       # scipy CSR [user_num, item_num] of positive values (clicks, play counts)
    svd = m.to_svd_model()                  # P = X, Q = Y as float32, mu = 0, biases = 0
    svd.recommend(users, 10, exclude=user_items)

    ImplicitALS(user_num, item_num, factors=128, solver="cg", cg_steps=3)      # conjugate gradient: factors up to 256

``solver="cholesky"`` (the default, factors up to 64) solves every row's normal equations exactly; ``solver="cg"`` takes
``cg_steps`` conjugate-gradient steps per row from the row as it stands and never forms a per-row matrix
(csrc/ials_cg.hip; the header states the solver).
Preference 1 on stored pairs and 0 elsewhere, confidence ``1 + alpha * value`` on stored pairs and 1 elsewhere; the fit
minimises ``sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + regularization (|X|^2 + |Y|^2)`` over all pairs (include/tfrecomm.h).
Serving goes through ``to_svd_model``: ``recommend``, ``rank_items``, ``similar_items`` and ``evaluate_ranking`` take the
``SvdModel`` it returns.

    rows = m.fold_in_users(new_user_items)                  # [n, item_num] lists the model never saw -> [n, factors]
    m.partial_fit_users(userids, their_new_lists)           # the same, written into rows of the user factors
    svd = m.to_svd_model(extra_users=256)
    items, scores = m.recommend_lists(svd, new_user_items, k=10)    # fold in, cast and top-K without leaving the device

Fold-in solves one row of a half-sweep per given list with the half-sweep's own kernels (include/tfrecomm.h
tfr_ials_fold_in); ``fold_in_items`` / ``partial_fit_items`` are the item side.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


class ImplicitALS(object):
    def __init__(self, user_num, item_num, factors=32, regularization=0.01, alpha=40.0, iterations=15, device=0, chunk=512,
                 solver="cholesky", cg_steps=3):
        self.user_num, self.item_num, self.factors = int(user_num), int(item_num), int(factors)
        self.regularization, self.alpha, self.iterations = float(regularization), float(alpha), int(iterations)
        self.device, self.chunk = int(device), int(chunk)
        if solver not in ("cholesky", "cg"):
            raise ValueError("solver must be 'cholesky' or 'cg', got %r" % (solver,))
        self.solver, self.cg_steps = solver, int(cg_steps)
        self.sweep_ms = 0.0
        self.fold_ms = 0.0                                 # device time of the last fold-in
        self._lib = L.load()
        self._h = L._p()
        if solver == "cg":
            self._check(self._lib.tfr_ials_create_cg(C.byref(self._h), self.user_num, self.item_num, self.factors,
                                                     self.regularization, self.alpha, self.cg_steps, self.device))
        else:
            self._check(self._lib.tfr_ials_create(C.byref(self._h), self.user_num, self.item_num, self.factors, self.regularization,
                                                  self.alpha, self.device))

    def _check(self, rc):
        if rc != L.OK:
            text = self._lib.tfr_ials_last_error().decode("utf-8", "replace")
            raise (L.OutOfRangeError if rc == L.ERR_OOB else L.TfrError)(rc, text)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.tfr_ials_destroy(self._h)
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

    @staticmethod
    def _p64(a):
        return None if a is None else a.ctypes.data_as(L._f64p)

    # -- data and factors -----------------------------------------------------------
    def load(self, user_items):
        """``user_items``: scipy sparse [user_num, item_num]; duplicates are summed and rows sorted first (as
        ``rated_matrix`` does).  Values must be positive and finite.  A second load replaces the first."""
        x = user_items.tocsr().astype(np.float64)          # a copy: the caller's matrix is left as it is
        if x.shape != (self.user_num, self.item_num):
            raise ValueError("user_items must be [%d, %d], got %s" % (self.user_num, self.item_num, x.shape))
        x.sum_duplicates()
        x.sort_indices()
        indptr = np.ascontiguousarray(x.indptr, np.int64)
        items = np.ascontiguousarray(x.indices, np.int32)
        vals = np.ascontiguousarray(x.data, np.float64)
        self._check(self._lib.tfr_ials_load(self._h, L.ptr_i64(indptr), L.ptr_i32(items), self._p64(vals), self.chunk))

    def init_factors(self, seed=0, stddev=0.01):
        """X then Y from ``RandomState(seed).normal(0, stddev)``, drawn on the host"""
        rs = np.random.RandomState(seed)
        X = rs.normal(0.0, stddev, (self.user_num, self.factors))
        Y = rs.normal(0.0, stddev, (self.item_num, self.factors))
        self.set_factors(X, Y)

    def set_factors(self, X=None, Y=None):
        tabs = []
        for a, rows in ((X, self.user_num), (Y, self.item_num)):
            if a is not None:
                a = np.ascontiguousarray(a, np.float64)
                if a.shape != (rows, self.factors):
                    raise ValueError("factors must be [%d, %d], got %s" % (rows, self.factors, a.shape))
            tabs.append(a)
        self._check(self._lib.tfr_ials_set(self._h, self._p64(tabs[0]), self._p64(tabs[1])))

    @property
    def user_factors(self):
        X = np.empty((self.user_num, self.factors), np.float64)
        self._check(self._lib.tfr_ials_get(self._h, self._p64(X), None))
        return X

    @property
    def item_factors(self):
        Y = np.empty((self.item_num, self.factors), np.float64)
        self._check(self._lib.tfr_ials_get(self._h, None, self._p64(Y)))
        return Y

    # -- training -------------------------------------------------------------------
    def half_sweep(self, side):
        """every user (side 0) or every item (side 1) solved from the other side's factors; returns the device time in ms"""
        ms = C.c_float()
        self._check(self._lib.tfr_ials_half(self._h, int(side), C.byref(ms)))
        self.sweep_ms += ms.value
        return ms.value

    def sweep(self, n=1):
        """n x (users, then items)"""
        ms = C.c_float()
        self._check(self._lib.tfr_ials_sweep(self._h, int(n), C.byref(ms)))
        self.sweep_ms += ms.value
        return ms.value

    def fit(self, user_items, seed=0):
        self.load(user_items)
        self.init_factors(seed)
        self.sweep_ms = 0.0
        self.sweep(self.iterations)
        return self

    def loss(self):
        out = C.c_double()
        self._check(self._lib.tfr_ials_loss(self._h, C.byref(out)))
        return out.value

    def gram(self, side):
        """T^T T of the user (side 0) or item (side 1) factors, as the other side's half-sweep computes it"""
        G = np.empty((self.factors, self.factors), np.float64)
        self._check(self._lib.tfr_ials_gram(self._h, int(side), self._p64(G)))
        return G

    # -- fold-in: rows for lists the model does not hold (include/tfrecomm.h tfr_ials_fold_in) ------------------
    def _lists(self, lists, n_other, what):
        """prepared as ``load`` prepares its matrix: a float64 CSR copy, duplicates summed, rows sorted"""
        x = lists.tocsr().astype(np.float64)
        if x.ndim != 2 or x.shape[1] != n_other:
            raise ValueError("%s must be [n, %d], got %s" % (what, n_other, x.shape))
        x.sum_duplicates()
        x.sort_indices()
        return x

    def _fold_in(self, side, x, rows=None, start=None, want=True):
        n = x.shape[0]
        indptr = np.ascontiguousarray(x.indptr, np.int64)
        ids = np.ascontiguousarray(x.indices, np.int32)
        vals = np.ascontiguousarray(x.data, np.float64)
        if start is not None:
            start = np.ascontiguousarray(start, np.float64)
            if start.shape != (n, self.factors):
                raise ValueError("start must be [%d, %d], got %s" % (n, self.factors, start.shape))
        out = np.empty((n, self.factors), np.float64) if want else None
        ms = C.c_float()
        self._check(self._lib.tfr_ials_fold_in(self._h, side, n, L.ptr_i64(indptr), L.ptr_i32(ids), self._p64(vals), self.chunk,
                                               None if rows is None else L.ptr_i32(rows), self._p64(start), self._p64(out),
                                               C.byref(ms)))
        self.fold_ms = ms.value
        return out

    def fold_in_users(self, user_items, start=None):
        """The factor rows of ``n`` users the model does not hold, from their item lists: ``user_items`` is a scipy sparse
        ``[n, item_num]`` of positive values (prepared as ``load`` does: a copy, duplicates summed, rows sorted).  Row ``e`` is
        what a user half-sweep would give a user with list ``e``, from the item factors as they stand; an empty list gives
        zeros.  ``start`` ``[n, factors]``: where the conjugate-gradient solver starts (``solver="cg"`` only; default 0).
        Returns ``[n, factors]`` float64.  Nothing in the model changes; no ``load`` is needed."""
        return self._fold_in(0, self._lists(user_items, self.item_num, "user_items"), start=start)

    def fold_in_items(self, item_users, start=None):
        """``fold_in_users`` for new items: ``item_users`` is ``[n, user_num]``, row ``e`` the users of item ``e``"""
        return self._fold_in(1, self._lists(item_users, self.user_num, "item_users"), start=start)

    def _partial_fit(self, side, ids, x, what):
        rows = np.ascontiguousarray(L.as_i32(ids, what)).reshape(-1)
        if rows.size != x.shape[0]:
            raise ValueError("%d %s for %d lists" % (rows.size, what, x.shape[0]))
        if np.unique(rows).size != rows.size:
            raise ValueError("%s repeat an id" % what)
        self._fold_in(side, x, rows=rows, want=False)

    def partial_fit_users(self, userids, user_items):
        """Rows ``userids`` of the user factors recomputed in place from the lists ``user_items`` ``[len(userids), item_num]``
        (``fold_in_users`` written into those rows; ``solver="cg"`` starts from the rows as they stand).  Duplicate ids raise
        ``ValueError``.  The resident lists are NOT changed: a later ``sweep`` still solves every user from what ``load``
        gave it, these users included."""
        self._partial_fit(0, userids, self._lists(user_items, self.item_num, "user_items"), "userids")

    def partial_fit_items(self, itemids, item_users):
        """``partial_fit_users`` for rows ``itemids`` of the item factors, from ``item_users`` ``[len(itemids), user_num]``.
        The resident lists are not changed either."""
        self._partial_fit(1, itemids, self._lists(item_users, self.user_num, "item_users"), "itemids")

    # -- serving --------------------------------------------------------------------
    def to_svd_model(self, extra_users=0, **svd_opts):
        """An ``SvdModel(user_num + extra_users, item_num, factors)`` with P = X and Q = Y cast to float32, mu = 0 and zero
        biases: its score is the dot product.  The ``extra_users`` rows after the fitted ones are zero: guest rows for
        ``recommend_lists``.  Copies through the host."""
        from .engine import SvdModel
        extra_users = int(extra_users)
        if extra_users < 0:
            raise ValueError("extra_users must not be negative")
        svd_opts.setdefault("device", self.device)
        users = self.user_num + extra_users
        m = SvdModel(users, self.item_num, self.factors, **svd_opts)
        P = np.zeros((users, self.factors), np.float32)
        P[:self.user_num] = self.user_factors
        m.set_tables(np.float32(0.0), np.zeros(users, np.float32), np.zeros(self.item_num, np.float32),
                     P, self.item_factors.astype(np.float32))
        return m

    def recommend_lists(self, svd, user_items, k=10, exclude=True, return_scores=True):
        """Top-``k`` for users known only by their lists.  ``svd``: this model's ``to_svd_model(extra_users=g)``, ``g`` > 0.
        The lists ``user_items`` ``[n, item_num]`` are folded in, their rows written as float32 into ``svd``'s guest rows on
        the device (no host copy of any table) and ``svd.recommend`` asked for those rows, ``g`` lists at a time; with
        ``exclude`` each list's own items are left out.  Returns what ``recommend`` returns, one row per list."""
        guests = svd.user_num - self.user_num
        if guests <= 0:
            raise ValueError("svd has no guest rows: make it with to_svd_model(extra_users=...)")
        if (svd.item_num, svd.dim, svd.device) != (self.item_num, self.factors, self.device):
            raise ValueError("svd is not this model's to_svd_model()")
        x = self._lists(user_items, self.item_num, "user_items")
        n, k = x.shape[0], int(k)
        items = np.empty((n, k), np.int32)
        scores = np.empty((n, k), np.float32) if return_scores else None
        if n:
            self._fold_in(0, x, want=False)
        users = np.arange(self.user_num, svd.user_num, dtype=np.int32)
        for lo in range(0, n, guests):
            cnt = min(guests, n - lo)
            base, _ = svd.table_devptr(L.P)
            self._check(self._lib.tfr_ials_export_f32(self._h, 2, lo, cnt, base + 4 * self.user_num * self.factors))
            p = x.indptr[lo:lo + cnt + 1]
            excl = (p - p[0], x.indices[p[0]:p[-1]]) if exclude else None
            got = svd.recommend(users[:cnt], k, exclude=excl, return_scores=return_scores)
            if return_scores:
                items[lo:lo + cnt], scores[lo:lo + cnt] = got
            else:
                items[lo:lo + cnt] = got
        return (items, scores) if return_scores else items
