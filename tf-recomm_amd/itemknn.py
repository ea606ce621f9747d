"""``ItemKNN``: item-based nearest neighbours from the interaction matrix itself, fitted and served on the GPU
(csrc/itemknn.hip; include/tfrecomm.h states the model).

    knn = ItemKNN(user_num, item_num, K=20, metric="cosine", shrink=0.0)
    knn.fit(user_items)                              # scipy CSR [user_num, item_num]; the pattern counts, values do not
    nb, sim = knn.neighbours()                       # [item_num, K] each, -1 / -inf past an item's co-rated items
    items, scores = knn.recommend(users, 10, exclude=user_items)
    evaluate_ranking(knn, test_users, test_items, exclude=user_items)

``c_ij`` = users with both items, ``n_i`` = users of item ``i``; ``cosine`` is ``c / (sqrt(n_i n_j) + shrink)``, ``jaccard``
``c / (n_i + n_j - c + shrink)``, ``count`` ``c``, each computed in float64 and rounded once to float32.  An item keeps its
``K`` best neighbours (similarity descending, then id ascending).  A user's score of item ``j`` is the float32 sum, over the
user's items ``i`` ascending, of ``sim(i, j)`` where ``j`` is among ``i``'s kept neighbours; every item is a candidate and one
without evidence scores 0.  ``recommend`` and ``rank_items`` follow ``SvdModel``'s contracts on these scores.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import exclusion_csr, rank_call

METRIC = {"cosine": 0, "jaccard": 1, "count": 2}


def plan(item_num, k, n_rows, which):
    """What the fit (``which`` 0: ``k`` is K, ``n_rows`` the items) or the scoring launch (``which`` 1) will do, computed on
    the host without a device: a dict of ``width`` (columns per catalogue slice), ``slices``, ``chunk`` (rows per chunk),
    ``lds`` (bytes per workgroup) and ``ahead`` (list entries a wave loads ahead)."""
    w, s, a = C.c_int32(), C.c_int32(), C.c_int32()
    ch, lds = C.c_int64(), C.c_int64()
    lib = L.load()
    rc = lib.tfr_knn_plan(int(item_num), int(k), int(n_rows), int(which), C.byref(w), C.byref(s), C.byref(ch), C.byref(lds), C.byref(a))
    if rc != L.OK:
        raise L.TfrError(rc, lib.tfr_knn_last_error().decode("utf-8", "replace"))
    return dict(width=w.value, slices=s.value, chunk=ch.value, lds=lds.value, ahead=a.value)


def _pattern(user_items, n_cols, what):
    """(indptr int64, items int32) of a scipy sparse matrix's pattern - a copy with duplicates merged, explicit zeros dropped
    and rows sorted - or of an (indptr, items) pair, which goes to the library's checks as it is"""
    if isinstance(user_items, tuple):
        indptr, items = user_items
        indptr = np.ascontiguousarray(np.asarray(indptr, np.int64)).reshape(-1)
        items = L.as_i32(items, what).reshape(-1)
        if indptr.size < 1 or (indptr.size and indptr[-1] > items.size):
            raise ValueError("%s: indptr must hold n + 1 entries that stay inside the items" % what)
        return indptr, items
    x = user_items.tocsr().copy()
    if x.ndim != 2 or x.shape[1] != n_cols:
        raise ValueError("%s must be [n, %d], got %s" % (what, n_cols, x.shape))
    x.sum_duplicates()
    x.eliminate_zeros()
    x.sort_indices()
    return np.ascontiguousarray(x.indptr, np.int64), np.ascontiguousarray(x.indices, np.int32)


class ItemKNN(object):
    def __init__(self, user_num, item_num, K=20, metric="cosine", shrink=0.0, device=0):
        if metric not in METRIC:
            raise ValueError("metric must be one of %s, got %r" % (sorted(METRIC), metric))
        self.user_num, self.item_num, self.K = int(user_num), int(item_num), int(K)
        self.metric, self.shrink, self.device = metric, float(shrink), int(device)
        self.fit_ms = 0.0                                  # device time of the last fit
        self._nb = None                                    # host copy of the lists, fetched when first asked for
        self._lib = L.load()
        self._h = L._p()
        self._check(self._lib.tfr_knn_create(C.byref(self._h), self.user_num, self.item_num, self.K, METRIC[metric], self.shrink,
                                             self.device))

    def _check(self, rc):
        if rc != L.OK:
            text = self._lib.tfr_knn_last_error().decode("utf-8", "replace")
            raise (L.OutOfRangeError if rc == L.ERR_OOB else L.TfrError)(rc, text)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.tfr_knn_destroy(self._h)
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

    # -- data and neighbour lists -----------------------------------------------------
    def load(self, user_items):
        """``user_items``: scipy sparse [user_num, item_num] (its pattern: values are ignored, explicit zeros dropped) or an
        (indptr, items) pair with strictly increasing rows.  A second load replaces the first and forgets the lists."""
        indptr, items = _pattern(user_items, self.item_num, "user_items")
        if indptr.size != self.user_num + 1:
            raise ValueError("user_items must hold %d rows" % self.user_num)
        self._nb = None
        self._check(self._lib.tfr_knn_load(self._h, L.ptr_i64(indptr), L.ptr_i32(items)))

    def fit(self, user_items=None):
        """``load`` (when ``user_items`` is given), then the neighbour lists of every item, which stay on the device"""
        if user_items is not None:
            self.load(user_items)
        ms = C.c_float()
        self._nb = None
        self._check(self._lib.tfr_knn_fit(self._h, C.byref(ms)))
        self.fit_ms = ms.value
        return self

    def neighbours(self):
        """``(items int32 [item_num, K], scores float32 [item_num, K])``: best first, -1 / -inf past the co-rated items"""
        if self._nb is None:
            items = np.empty((self.item_num, self.K), np.int32)
            scores = np.empty((self.item_num, self.K), np.float32)
            self._check(self._lib.tfr_knn_get_neighbours(self._h, 0, self.item_num, L.ptr_i32(items), L.ptr_f32(scores)))
            self._nb = (items, scores)
        return self._nb

    def set_neighbours(self, items, scores):
        """The lists of every item from host arrays [item_num, K] (``neighbours()`` of a fitted model, or constructed ones):
        ids in [-1, item_num), -1 is padding, no row names itself or repeats an item, real ids carry finite scores."""
        items = np.ascontiguousarray(L.as_i32(items, "neighbour ids"))
        scores = L.as_f32(scores)
        if items.shape != (self.item_num, self.K) or scores.shape != items.shape:
            raise ValueError("items and scores must be [%d, %d]" % (self.item_num, self.K))
        self._nb = None
        self._check(self._lib.tfr_knn_set_neighbours(self._h, 0, self.item_num, L.ptr_i32(items), L.ptr_f32(scores)))

    def similar_items(self, items, k=None):
        """The first ``k <= K`` neighbours of each of ``items``: a slice of the fitted lists, no launch"""
        k = self.K if k is None else int(k)
        if k < 1 or k > self.K:
            raise ValueError("k must be in [1, K = %d]" % self.K)
        ids = L.as_i32(items, "item ids").reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= self.item_num):
            raise L.OutOfRangeError(L.ERR_OOB, "items outside [0, %d)" % self.item_num)
        nb, sc = self.neighbours()
        return nb[ids, :k].copy(), sc[ids, :k].copy()

    # -- serving ------------------------------------------------------------------------
    def recommend(self, users, k=10, exclude=None, return_scores=True):
        """The ``k`` best items of each of ``users`` (resident: their loaded rows are the lists), best first, equal scores by
        item id.  ``exclude`` as in ``SvdModel.recommend``.  Returns ``items`` int32 [n, k] (-1 past the eligible items) and,
        if asked, ``scores`` float32 [n, k] (-inf there)."""
        u = L.as_i32(users, "user ids").reshape(-1)
        xp, xi = exclusion_csr(exclude, u)
        items = np.empty((u.size, int(k)), np.int32)
        scores = np.empty((u.size, int(k)), np.float32) if return_scores else None
        self._check(self._lib.tfr_knn_topk(self._h, L.ptr_i32(u), u.size, int(k), None if xp is None else L.ptr_i64(xp),
                                           None if xi is None else L.ptr_i32(xi), L.ptr_i32(items),
                                           None if scores is None else L.ptr_f32(scores)))
        return (items, scores) if return_scores else items

    def recommend_lists(self, user_items, k=10, exclude=True, return_scores=True):
        """``recommend`` for users the model does not hold, known by their lists: ``user_items`` is a scipy sparse
        [n, item_num] or an (indptr, items) pair.  ``exclude``: True leaves out each list's own items, None / False nothing,
        anything else as in ``recommend`` (aligned with the lists)."""
        indptr, ids = _pattern(user_items, self.item_num, "user_items")
        n = indptr.size - 1
        if exclude is True:
            xp, xi = indptr, ids
        elif exclude is None or exclude is False:
            xp, xi = None, None
        else:
            xp, xi = exclusion_csr(exclude, np.arange(n))
        items = np.empty((n, int(k)), np.int32)
        scores = np.empty((n, int(k)), np.float32) if return_scores else None
        self._check(self._lib.tfr_knn_topk_lists(self._h, L.ptr_i64(indptr), L.ptr_i32(ids), n, int(k),
                                                 None if xp is None else L.ptr_i64(xp), None if xi is None else L.ptr_i32(xi),
                                                 L.ptr_i32(items), None if scores is None else L.ptr_f32(scores)))
        return (items, scores) if return_scores else items

    def rank_items(self, users, targets, exclude=None):
        """0-based rank of each target item of each of ``users`` among all items not in ``exclude``, by the keys of
        ``recommend``: ``rank < k`` exactly when ``recommend(users, k, exclude)`` holds the target, at that position; -1 for
        an excluded target.  Arguments and return value as ``SvdModel.rank_items``."""
        u = L.as_i32(users, "user ids").reshape(-1)

        def call(ip, it, xp, xi, out):
            self._check(self._lib.tfr_knn_rank_items(self._h, L.ptr_i32(u), u.size, ip, it, xp, xi, out))
        return rank_call(call, u, targets, exclude)
