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
from .item_lists import ItemListModel


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


class EASE(ItemListModel):
    _family = "ease"

    def __init__(self, user_num, item_num, regularization=500.0, device=0):
        self.user_num, self.item_num = int(user_num), int(item_num)
        self.regularization, self.device = float(regularization), int(device)
        self.fit_ms = 0.0                                  # device time of the last fit: Gram + inverse + weights
        self.fit_ms_parts = dict(gram=0.0, inverse=0.0, weights=0.0)
        self._f64_is = None                                # what the device's float64 buffer holds: None, "G" or "P"
        self._lib = L.load()
        self._h = L._p()
        self._check(self._lib.tfr_ease_create(C.byref(self._h), self.user_num, self.item_num, self.regularization, self.device))

    # -- data and fit -------------------------------------------------------------------
    def load(self, user_items):
        """``user_items``: scipy sparse [user_num, item_num] (its pattern: values are ignored, explicit zeros dropped) or an
        (indptr, items) pair with strictly increasing rows.  A second load replaces the first and forgets Gram and weights."""
        self._f64_is = None
        self._load(user_items)

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
