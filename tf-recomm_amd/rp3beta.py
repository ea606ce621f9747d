"""``WeightedItemKNN`` and ``RP3beta``: neighbour lists from a weighted co-occurrence, fitted on the GPU by
``tfr_knn_fit_weighted`` (csrc/itemknn.hip; include/tfrecomm.h states the model) and served as ``ItemKNN`` serves its own.

    rp3 = RP3beta(user_num, item_num, K=100, alpha=1.0, beta=0.6)        # beta=0: P3alpha
    rp3.fit(user_items)                              # scipy CSR [user_num, item_num]; the pattern counts, values do not
    items, scores = rp3.recommend(users, 10, exclude=user_items)
    evaluate_ranking(rp3, test_users, test_items, exclude=user_items)

The general form takes a weight ``w_u`` in [0, 1] per user and two non-negative float64 factors per item:

    q_u  = rint(w_u * 2^shift)                       uint64: the weight in fixed point
    S_ij = sum of q_u over the users with both i and j           an exact integer
    sim(i -> j) = float32(float64(S_ij) * 2^-shift * row_scale[i] * col_scale[j])

and an item keeps the ``K`` best ``j != i`` with ``S_ij > 0`` (similarity descending, then id ascending).  The diagonal is
left out by definition, as in ``ItemKNN``.  The sums are integers, so they do not depend on the order of the adds and a fit
repeats bit for bit.

RP3beta (Paudel et al. 2017; P3alpha, Cooper et al. 2014, at ``beta = 0``) is the two-step random walk item -> user -> item
with the popularity of the target divided out: ``w_u = deg(u)^-alpha``, ``row_scale[i] = n_i^-alpha``, ``col_scale[j] =
n_j^-beta``, 0 for empty users and items, all in NumPy float64.  **What is fitted is RP3beta with the user weights rounded to
multiples of 2^-shift.**  ``shift = min(40, 62 - bit_length(max_i n_i))`` keeps every sum below 2^62; each kept similarity
then lies within the relative distance ``2^-(shift+1) / min_u w_u + 2^-24 + (c_ij + 8) * 2^-53`` of the float64 formula
``diag(n^-alpha) X^T diag(d^-alpha) X diag(n^-beta)`` (one rounding per weight, the float32 rounding, the float64 chains of
both sides): at shift 40 and users of at most 1000 items with alpha 1 that is 6.0e-8, the float32 rounding itself.

TF-IDF neighbours on binary data are ``w_u = 1``, ``row_scale[i] = col_scale[i] = idf_i`` (the dot product of idf-weighted
columns; divide both by the column norm ``idf_i * sqrt(n_i)`` for the cosine).  BM25 on binary data has the per-entry weight
``idf_i * g_u`` with ``g_u = (k1 + 1) / (1 + k1 * (1 - b + b * deg(u) / avgdeg))``, an item factor times a user factor: it is
``w_u = (g_u / max g)^2``, ``row_scale[i] = idf_i * (max g)^2``, ``col_scale[j] = idf_j``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .item_lists import _pattern
from .itemknn import ItemKNN

SHIFT_MAX = 40


def weighted_plan(item_num, k, n_rows):
    """What the weighted fit will do (``k`` is K, ``n_rows`` the items), computed on the host without a device: the dict of
    ``itemknn.plan``"""
    w, s, a = C.c_int32(), C.c_int32(), C.c_int32()
    ch, lds = C.c_int64(), C.c_int64()
    lib = L.load()
    rc = lib.tfr_knn_weighted_plan(int(item_num), int(k), int(n_rows), C.byref(w), C.byref(s), C.byref(ch), C.byref(lds), C.byref(a))
    if rc != L.OK:
        raise L.TfrError(rc, lib.tfr_knn_last_error().decode("utf-8", "replace"))
    return dict(width=w.value, slices=s.value, chunk=ch.value, lds=lds.value, ahead=a.value)


def pick_shift(max_item_users):
    """the largest shift up to 40 at which ``max_item_users`` weights of 2^shift sum below 2^62"""
    return min(SHIFT_MAX, 62 - int(max_item_users).bit_length())


def quantise(weights, shift):
    """uint64 ``rint(w * 2^shift)`` of float weights in [0, 1]"""
    w = np.asarray(weights, np.float64).reshape(-1)
    if w.size and not (np.all(w >= 0.0) and np.all(w <= 1.0)):          # NaN fails both
        raise ValueError("user weights must lie in [0, 1]")
    return np.rint(w * np.float64(2.0 ** int(shift))).astype(np.uint64)


def _neg_power(counts, exponent):
    """float64 ``counts ** -exponent``, 0 where the count is 0"""
    n = np.asarray(counts, np.float64)
    return np.where(n > 0, np.power(np.maximum(n, 1.0), -np.float64(exponent)), 0.0)


class WeightedItemKNN(ItemKNN):
    """``ItemKNN`` whose lists come from the weighted fit; everything but ``fit`` is inherited"""

    def __init__(self, user_num, item_num, K=20, device=0):
        super().__init__(user_num, item_num, K=K, metric="count", shrink=0.0, device=device)
        self.q = None                                      # uint64 [user_num]: the weights the last fit used
        self.shift = None
        self._max_item_users = 0                           # of the loaded data

    def load(self, user_items):
        indptr, items = _pattern(user_items, self.item_num, "user_items")
        super().load((indptr, items))                      # the library checks the ids
        self._max_item_users = int(np.bincount(items).max()) if items.size else 0

    def fit(self, user_items, user_weights, row_scale, col_scale, shift=None):
        """``load`` (when ``user_items`` is not None), quantise ``user_weights`` (floats in [0, 1]) at ``shift`` (picked from
        the longest loaded item list when None), then the lists of every item"""
        if user_items is not None:
            self.load(user_items)
        shift = pick_shift(self._max_item_users) if shift is None else int(shift)
        return self.fit_raw(quantise(user_weights, shift), row_scale, col_scale, shift)

    def fit_raw(self, q, row_scale, col_scale, shift):
        """the C entry as it is: uint64 weights ``q``, float64 scales, ``shift`` in [0, 62], on the loaded data"""
        q = np.ascontiguousarray(np.asarray(q, np.uint64)).reshape(-1)
        rs = np.ascontiguousarray(np.asarray(row_scale, np.float64)).reshape(-1)
        cs = np.ascontiguousarray(np.asarray(col_scale, np.float64)).reshape(-1)
        if q.size != self.user_num or rs.size != self.item_num or cs.size != self.item_num:
            raise ValueError("need %d user weights and %d row and column scales" % (self.user_num, self.item_num))
        ms = C.c_float()
        self._nb = None
        self._check(self._lib.tfr_knn_fit_weighted(self._h, q.ctypes.data_as(C.POINTER(C.c_uint64)), rs.ctypes.data_as(L._f64p),
                                                   cs.ctypes.data_as(L._f64p), int(shift), C.byref(ms)))
        self.q, self.shift, self.fit_ms = q, int(shift), ms.value
        return self


class RP3beta(WeightedItemKNN):
    def __init__(self, user_num, item_num, K=100, alpha=1.0, beta=0.6, device=0):
        super().__init__(user_num, item_num, K=K, device=device)
        self.alpha, self.beta = float(alpha), float(beta)

    def fit(self, user_items):
        """``load``, then the lists of the model stated at the top of this module"""
        indptr, items = _pattern(user_items, self.item_num, "user_items")
        self.load((indptr, items))
        deg = np.diff(indptr)
        n = np.bincount(items, minlength=self.item_num)
        return super().fit(None, _neg_power(deg, self.alpha), _neg_power(n, self.alpha), _neg_power(n, self.beta))
