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
from .item_lists import ItemListModel

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


class ItemKNN(ItemListModel):
    _family = "knn"

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

    # -- data and neighbour lists -----------------------------------------------------
    def load(self, user_items):
        """``user_items``: scipy sparse [user_num, item_num] (its pattern: values are ignored, explicit zeros dropped) or an
        (indptr, items) pair with strictly increasing rows.  A second load replaces the first and forgets the lists."""
        self._nb = None
        self._load(user_items)

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
