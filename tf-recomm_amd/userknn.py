"""``UserKNN``: user-based nearest neighbours from the interaction matrix itself, fitted and served on the GPU
(csrc/userknn.hip; include/tfrecomm.h states the model).

    knn = UserKNN(user_num, item_num, K=50, metric="cosine", shrink=0.0)
    knn.fit(user_items)                              # scipy CSR [user_num, item_num]; the pattern counts, values do not
    nb, sim = knn.neighbours()                       # [user_num, K] each, -1 / -inf past a user's co-raters
    items, scores = knn.recommend(users, 10, exclude=user_items)
    items, scores = knn.recommend_lists(new_rows, 10)    # users the model does not hold: neighbours found at query time
    evaluate_ranking(knn, test_users, test_items, exclude=user_items)

``c_uv`` = items both users have, ``d_u`` = items of user ``u``; ``cosine`` is ``c / (sqrt(d_u d_v) + shrink)``, ``jaccard``
``c / (d_u + d_v - c + shrink)``, ``count`` ``c``, each computed in float64 and rounded once to float32, as ``ItemKNN`` does
on the other orientation.  A user keeps its ``K`` best neighbours (similarity descending, then id ascending).  A user's score
of item ``j`` is the float32 sum, over the user's neighbours in list order, of the similarities of those who have ``j``; every
item is a candidate and one without evidence scores 0.  The sum is not divided by the sum of the similarities: a constant per
user moves no ranking, and without it the score is a pure sum of the stored float32 values.  ``recommend_lists`` needs only
``load``: it finds each list's neighbours among the loaded users (a loaded user with the same row is simply the best one) and
ignores fitted or set lists.  ``recommend`` and ``rank_items`` follow ``SvdModel``'s contracts on these scores.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .item_lists import ItemListModel
from .itemknn import METRIC


def plan(n_cols, k, n_rows, which):
    """What the fit (``which`` 0: ``n_cols`` the users, ``k`` is K, ``n_rows`` the users), the scoring launch (``which`` 1:
    ``n_cols`` the items, ``n_rows`` the queries) or the neighbour search of query lists (``which`` 2: ``n_cols`` the users,
    ``k`` is K, ``n_rows`` the lists) will do, computed on the host without a device: a dict of ``width`` (columns per
    slice), ``slices``, ``chunk`` (rows per chunk), ``lds`` (bytes per workgroup) and ``ahead`` (list entries a wave takes at
    once)."""
    w, s, a = C.c_int32(), C.c_int32(), C.c_int32()
    ch, lds = C.c_int64(), C.c_int64()
    lib = L.load()
    rc = lib.tfr_uknn_plan(int(n_cols), int(k), int(n_rows), int(which), C.byref(w), C.byref(s), C.byref(ch), C.byref(lds), C.byref(a))
    if rc != L.OK:
        raise L.TfrError(rc, lib.tfr_uknn_last_error().decode("utf-8", "replace"))
    return dict(width=w.value, slices=s.value, chunk=ch.value, lds=lds.value, ahead=a.value)


class UserKNN(ItemListModel):
    _family = "uknn"

    def __init__(self, user_num, item_num, K=50, metric="cosine", shrink=0.0, device=0):
        if metric not in METRIC:
            raise ValueError("metric must be one of %s, got %r" % (sorted(METRIC), metric))
        self.user_num, self.item_num, self.K = int(user_num), int(item_num), int(K)
        self.metric, self.shrink, self.device = metric, float(shrink), int(device)
        self.fit_ms = 0.0                                  # device time of the last fit
        self._nb = None                                    # host copy of the lists, fetched when first asked for
        self._lib = L.load()
        self._h = L._p()
        self._check(self._lib.tfr_uknn_create(C.byref(self._h), self.user_num, self.item_num, self.K, METRIC[metric], self.shrink,
                                              self.device))

    # -- data and neighbour lists -----------------------------------------------------
    def load(self, user_items):
        """``user_items``: scipy sparse [user_num, item_num] (its pattern: values are ignored, explicit zeros dropped) or an
        (indptr, items) pair with strictly increasing rows.  A second load replaces the first and forgets the lists."""
        self._nb = None
        self._load(user_items)

    def fit(self, user_items=None):
        """``load`` (when ``user_items`` is given), then the neighbour lists of every user, which stay on the device"""
        if user_items is not None:
            self.load(user_items)
        ms = C.c_float()
        self._nb = None
        self._check(self._lib.tfr_uknn_fit(self._h, C.byref(ms)))
        self.fit_ms = ms.value
        return self

    def neighbours(self):
        """``(users int32 [user_num, K], scores float32 [user_num, K])``: best first, -1 / -inf past the co-raters"""
        if self._nb is None:
            users = np.empty((self.user_num, self.K), np.int32)
            scores = np.empty((self.user_num, self.K), np.float32)
            self._check(self._lib.tfr_uknn_get_neighbours(self._h, 0, self.user_num, L.ptr_i32(users), L.ptr_f32(scores)))
            self._nb = (users, scores)
        return self._nb

    def set_neighbours(self, users, scores):
        """The lists of every user from host arrays [user_num, K] (``neighbours()`` of a fitted model, or constructed ones):
        ids in [-1, user_num), -1 is padding, no row names itself or repeats a user, real ids carry finite scores."""
        users = np.ascontiguousarray(L.as_i32(users, "neighbour ids"))
        scores = L.as_f32(scores)
        if users.shape != (self.user_num, self.K) or scores.shape != users.shape:
            raise ValueError("users and scores must be [%d, %d]" % (self.user_num, self.K))
        self._nb = None
        self._check(self._lib.tfr_uknn_set_neighbours(self._h, 0, self.user_num, L.ptr_i32(users), L.ptr_f32(scores)))

    def similar_users(self, users, k=None):
        """The first ``k <= K`` neighbours of each of ``users``: a slice of the fitted lists, no launch"""
        k = self.K if k is None else int(k)
        if k < 1 or k > self.K:
            raise ValueError("k must be in [1, K = %d]" % self.K)
        ids = L.as_i32(users, "user ids").reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= self.user_num):
            raise L.OutOfRangeError(L.ERR_OOB, "users outside [0, %d)" % self.user_num)
        nb, sc = self.neighbours()
        return nb[ids, :k].copy(), sc[ids, :k].copy()
