"""``EASE``: Steck's embarrassingly shallow autoencoder, an item x item model in closed form, fitted and served on the GPU
(csrc/ease.hip; include/tfrecomm.h states the model).

    ease = EASE(user_num, item_num, regularization=500.0)
    ease.fit(user_items)                             # scipy CSR [user_num, item_num]; the pattern counts, values do not
    B = ease.weights()                               # float32 [item_num, item_num], zero diagonal
    items, scores = ease.recommend(users, 10, exclude=user_items)
    items, scores = ease.recommend_lists(new_user_items, 10)       # users the model has never seen, from their lists
    evaluate_ranking(ease, test_users, test_items, exclude=user_items)

``G = X^T X + regularization * I`` in float64 (exact integer co-counts), ``P = G^-1`` by a blocked Cholesky factorisation in
float64, ``B = -P / diag(P)`` column-wise, rounded once to float32, with a zero diagonal.  A user's score of item ``j`` is the
float32 sum, over the user's items ``i`` ascending, of ``B[i, j]``; every item is a candidate.  ``recommend`` and
``rank_items`` follow ``SvdModel``'s contracts on these scores.  The dense matrices cap the catalogue at 32768 items.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import exclusion_csr, rank_call
from .itemknn import _pattern


def plan(item_num, k=1, n_rows=0, which=0):
    """What the fit (``which`` 0) or the scoring launch (``which`` 1: ``n_rows`` queries for ``k``) will do, computed on the
    host without a device: a dict of ``nb`` (factorisation block), ``tile`` (results per side of the update kernel's MFMA
    tile), ``lds`` (bytes per workgroup), ``f64_bytes`` / ``f32_bytes`` (what a fit allocates), ``width`` (columns per
    catalogue slice), ``slices``, ``chunk`` (queries per chunk) and ``ahead`` (list items a wave loads ahead)."""
    nb, tile, w, s, a = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    lds, f64, f32, ch = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    lib = L.load()
    rc = lib.tfr_ease_plan(int(item_num), int(k), int(n_rows), int(which), C.byref(nb), C.byref(tile), C.byref(lds), C.byref(f64),
                           C.byref(f32), C.byref(w), C.byref(s), C.byref(ch), C.byref(a))
    if rc != L.OK:
        raise L.TfrError(rc, lib.tfr_ease_last_error().decode("utf-8", "replace"))
    return dict(nb=nb.value, tile=tile.value, lds=lds.value, f64_bytes=f64.value, f32_bytes=f32.value, width=w.value,
                slices=s.value, chunk=ch.value, ahead=a.value)


class EASE(object):
    def __init__(self, user_num, item_num, regularization=500.0, device=0):
        self.user_num, self.item_num = int(user_num), int(item_num)
        self.regularization, self.device = float(regularization), int(device)
        self.fit_ms = 0.0                                  # device time of the last fit: Gram + inverse + weights
        self.fit_ms_parts = dict(gram=0.0, inverse=0.0, weights=0.0)
        self._f64_is = None                                # what the device's float64 buffer holds: None, "G" or "P"
        self._lib = L.load()
        self._h = L._p()
        self._check(self._lib.tfr_ease_create(C.byref(self._h), self.user_num, self.item_num, self.regularization, self.device))

    def _check(self, rc):
        if rc != L.OK:
            text = self._lib.tfr_ease_last_error().decode("utf-8", "replace")
            raise (L.OutOfRangeError if rc == L.ERR_OOB else L.TfrError)(rc, text)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.tfr_ease_destroy(self._h)
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

    # -- data and fit -------------------------------------------------------------------
    def load(self, user_items):
        """``user_items``: scipy sparse [user_num, item_num] (its pattern: values are ignored, explicit zeros dropped) or an
        (indptr, items) pair with strictly increasing rows.  A second load replaces the first and forgets Gram and weights."""
        indptr, items = _pattern(user_items, self.item_num, "user_items")
        if indptr.size != self.user_num + 1:
            raise ValueError("user_items must hold %d rows" % self.user_num)
        self._f64_is = None
        self._check(self._lib.tfr_ease_load(self._h, L.ptr_i64(indptr), L.ptr_i32(items)))

    def _solve(self, keep_inverse):
        ms = (C.c_float * 3)()
        self._f64_is = None
        self._check(self._lib.tfr_ease_solve(self._h, 1 if keep_inverse else 0, ms))
        self._f64_is = "P" if keep_inverse else None
        self.fit_ms_parts = dict(gram=ms[0], inverse=ms[1], weights=ms[2])
        self.fit_ms = float(ms[0] + ms[1] + ms[2])
        return self

    def build_gram(self):
        """``G = X^T X + regularization * I`` of the loaded pattern into the device's float64 buffer"""
        self._f64_is = None
        self._check(self._lib.tfr_ease_gram(self._h))
        self._f64_is = "G"
        return self

    def fit(self, user_items=None, keep_inverse=False):
        """``load`` (when ``user_items`` is given), the Gram matrix, its inverse and the weights, which stay on the device.
        ``keep_inverse`` keeps ``P`` for ``inverse()``; otherwise the float64 buffer is freed."""
        if user_items is not None:
            self.load(user_items)
        self.build_gram()
        return self._solve(keep_inverse)

    def fit_gram(self, G, keep_inverse=False):
        """the fit from a caller's Gram matrix, float64 [item_num, item_num]: finite, symmetric bit for bit, positive
        diagonal.  ``regularization`` is not added to it."""
        self.set_gram(G)
        return self._solve(keep_inverse)

    def set_gram(self, G):
        G = np.ascontiguousarray(np.asarray(G, np.float64))
        if G.shape != (self.item_num, self.item_num):
            raise ValueError("G must be [%d, %d]" % (self.item_num, self.item_num))
        self._f64_is = None
        self._check(self._lib.tfr_ease_set_gram(self._h, G.ctypes.data_as(L._f64p)))
        self._f64_is = "G"
        return self

    def _f64(self):
        out = np.empty((self.item_num, self.item_num), np.float64)
        self._check(self._lib.tfr_ease_get_f64(self._h, 0, self.item_num, out.ctypes.data_as(L._f64p)))
        return out

    def gram(self):
        """``G`` float64 [item_num, item_num]: the device's float64 buffer if it holds a Gram matrix (``build_gram`` /
        ``set_gram`` before the solve), else built from the loaded pattern first"""
        if self._f64_is != "G":
            self.build_gram()
        return self._f64()

    def inverse(self):
        """``P`` float64 [item_num, item_num], kept by a fit with ``keep_inverse``"""
        if self._f64_is != "P":
            raise L.TfrError(L.ERR_STATE, "no inverse: fit with keep_inverse=True")
        return self._f64()

    def weights(self):
        """``B`` float32 [item_num, item_num]"""
        out = np.empty((self.item_num, self.item_num), np.float32)
        self._check(self._lib.tfr_ease_get_weights(self._h, 0, self.item_num, L.ptr_f32(out)))
        return out

    def set_weights(self, B):
        """``B`` of every item from a host array (``weights()`` of a fitted model, or constructed): finite float32"""
        B = L.as_f32(B)
        if B.shape != (self.item_num, self.item_num):
            raise ValueError("B must be [%d, %d]" % (self.item_num, self.item_num))
        self._check(self._lib.tfr_ease_set_weights(self._h, 0, self.item_num, L.ptr_f32(B)))

    # -- serving ------------------------------------------------------------------------
    def recommend(self, users, k=10, exclude=None, return_scores=True):
        """The ``k`` best items of each of ``users`` (resident: their loaded rows are the lists), best first, equal scores by
        item id.  ``exclude`` as in ``SvdModel.recommend``.  Returns ``items`` int32 [n, k] (-1 past the eligible items) and,
        if asked, ``scores`` float32 [n, k] (-inf there)."""
        u = L.as_i32(users, "user ids").reshape(-1)
        xp, xi = exclusion_csr(exclude, u)
        items = np.empty((u.size, int(k)), np.int32)
        scores = np.empty((u.size, int(k)), np.float32) if return_scores else None
        self._check(self._lib.tfr_ease_topk(self._h, L.ptr_i32(u), u.size, int(k), None if xp is None else L.ptr_i64(xp),
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
        self._check(self._lib.tfr_ease_topk_lists(self._h, L.ptr_i64(indptr), L.ptr_i32(ids), n, int(k),
                                                  None if xp is None else L.ptr_i64(xp), None if xi is None else L.ptr_i32(xi),
                                                  L.ptr_i32(items), None if scores is None else L.ptr_f32(scores)))
        return (items, scores) if return_scores else items

    def rank_items(self, users, targets, exclude=None):
        """0-based rank of each target item of each of ``users`` among all items not in ``exclude``, by the keys of
        ``recommend``: ``rank < k`` exactly when ``recommend(users, k, exclude)`` holds the target, at that position; -1 for
        an excluded target.  Arguments and return value as ``SvdModel.rank_items``."""
        u = L.as_i32(users, "user ids").reshape(-1)

        def call(ip, it, xp, xi, out):
            self._check(self._lib.tfr_ease_rank_items(self._h, L.ptr_i32(u), u.size, ip, it, xp, xi, out))
        return rank_call(call, u, targets, exclude)
