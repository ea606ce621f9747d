"""``SLIM``: Ning & Karypis' sparse linear method, one elastic-net regression per item, fitted and served on the GPU
(csrc/slim.hip; include/tfrecomm.h states the model and the solver's order).

    slim = SLIM(user_num, item_num, l1=1.0, l2=5.0)
    slim.fit(user_items)                             # scipy CSR [user_num, item_num]; the pattern counts, values do not
    W = slim.weights()                               # float32 [item_num, item_num], zero diagonal, non-negative, sparse
    slim.sweeps(), slim.updates(), slim.converged()  # per item column
    items, scores = slim.recommend(users, 10, exclude=user_items)
    evaluate_ranking(slim, test_users, test_items, exclude=user_items)

``A = X^T X + l2 * I`` in float64 (exact integer co-counts).  Column ``j`` of ``W`` minimises
``1/2 w^T A w - a_j^T w + l1 * sum|w|`` with ``w[j] = 0`` and, when ``positive``, ``w >= 0``, by cyclic coordinate descent in
float64, at most ``max_iter`` sweeps, stopped when a sweep's largest change is at most ``tol * max|w|``.  In sklearn's
``ElasticNet(alpha, l1_ratio)`` terms over the ``user_num`` users: ``l1 = user_num * alpha * l1_ratio`` and
``l2 = user_num * alpha * (1 - l1_ratio)``.  Scores, ``recommend`` and ``rank_items`` are ``EASE``'s on ``W``.  A column's
state lives in one workgroup's LDS, which caps the catalogue at 16384 items.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .item_lists import ItemListModel


def plan(item_num, k=1, n_rows=0, which=0):
    """What the fit (``which`` 0) or the scoring launch (``which`` 1: ``n_rows`` queries for ``k``) will do, computed on the
    host without a device: a dict of ``window`` (coordinates the solver examines at once = threads per workgroup), ``grid``
    (solver workgroups; columns past it are taken in strides), ``lds`` (bytes per workgroup), ``w_in_lds`` (whether a
    column's weights live in LDS beside its residual; False: in a global scratch row per workgroup), ``f64_bytes`` /
    ``f32_bytes`` (what a fit allocates) and EASE's scoring slicing: ``width``, ``slices``, ``chunk``, ``ahead``."""
    t, g, wl, w, s, a = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    lds, f64, f32, ch = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    lib = L.load()
    rc = lib.tfr_slim_plan(int(item_num), int(k), int(n_rows), int(which), C.byref(t), C.byref(g), C.byref(lds), C.byref(wl),
                           C.byref(f64), C.byref(f32), C.byref(w), C.byref(s), C.byref(ch), C.byref(a))
    if rc != L.OK:
        raise L.TfrError(rc, lib.tfr_slim_last_error().decode("utf-8", "replace"))
    return dict(window=t.value, grid=g.value, lds=lds.value, w_in_lds=bool(wl.value), f64_bytes=f64.value, f32_bytes=f32.value,
                width=w.value, slices=s.value, chunk=ch.value, ahead=a.value)


class SLIM(ItemListModel):
    _family = "slim"

    def __init__(self, user_num, item_num, l1=1.0, l2=5.0, positive=True, max_iter=100, tol=1e-4, device=0):
        self.user_num, self.item_num = int(user_num), int(item_num)
        self.l1, self.l2, self.positive = float(l1), float(l2), bool(positive)
        self.max_iter, self.tol, self.device = int(max_iter), float(tol), int(device)
        self.fit_ms = 0.0                                  # device time of the last fit: Gram + solve
        self.fit_ms_parts = dict(gram=0.0, solve=0.0)
        self._has_gram = False
        self._lib = L.load()
        self._h = L._p()
        self._check(self._lib.tfr_slim_create(C.byref(self._h), self.user_num, self.item_num, self.l2, self.device))

    # -- data and fit -------------------------------------------------------------------
    def load(self, user_items):
        """``user_items``: scipy sparse [user_num, item_num] (its pattern: values are ignored, explicit zeros dropped) or an
        (indptr, items) pair with strictly increasing rows.  A second load replaces the first and forgets Gram and weights."""
        self._has_gram = False
        self._load(user_items)

    def solve(self):
        """the solve alone, on the Gram matrix the device holds, with the attributes of the moment"""
        ms = (C.c_float * 2)()
        self._check(self._lib.tfr_slim_solve(self._h, self.l1, 1 if self.positive else 0, self.max_iter, self.tol, ms))
        self.fit_ms_parts = dict(gram=ms[0], solve=ms[1])
        self.fit_ms = float(ms[0] + ms[1])
        return self

    def build_gram(self):
        """``A = X^T X + l2 * I`` of the loaded pattern into the device's float64 buffer"""
        self._has_gram = False
        self._check(self._lib.tfr_slim_gram(self._h))
        self._has_gram = True
        return self

    def fit(self, user_items=None):
        """``load`` (when ``user_items`` is given), the Gram matrix and the solve.  The weights and the Gram matrix stay on
        the device: after a change of ``l1`` / ``positive`` / ``max_iter`` / ``tol``, ``solve()`` alone refits."""
        if user_items is not None:
            self.load(user_items)
        self.build_gram()
        return self.solve()

    def fit_gram(self, A):
        """the fit from a caller's Gram matrix, float64 [item_num, item_num]: finite and symmetric bit for bit.  ``l2`` is
        not added to it."""
        self.set_gram(A)
        return self.solve()

    def set_gram(self, A):
        A = np.ascontiguousarray(np.asarray(A, np.float64))
        if A.shape != (self.item_num, self.item_num):
            raise ValueError("A must be [%d, %d]" % (self.item_num, self.item_num))
        self._has_gram = False
        self._check(self._lib.tfr_slim_set_gram(self._h, A.ctypes.data_as(L._f64p)))
        self._has_gram = True
        return self

    def gram(self):
        """``A`` float64 [item_num, item_num]: the device's matrix if it holds one, else built from the loaded pattern first"""
        if not self._has_gram:
            self.build_gram()
        out = np.empty((self.item_num, self.item_num), np.float64)
        self._check(self._lib.tfr_slim_get_gram(self._h, 0, self.item_num, out.ctypes.data_as(L._f64p)))
        return out

    def weights(self):
        """``W`` float32 [item_num, item_num]"""
        out = np.empty((self.item_num, self.item_num), np.float32)
        self._check(self._lib.tfr_slim_get_weights(self._h, 0, self.item_num, L.ptr_f32(out)))
        return out

    def set_weights(self, W):
        """``W`` of every item from a host array (``weights()`` of a fitted model, or constructed): finite float32"""
        W = L.as_f32(W)
        if W.shape != (self.item_num, self.item_num):
            raise ValueError("W must be [%d, %d]" % (self.item_num, self.item_num))
        self._check(self._lib.tfr_slim_set_weights(self._h, 0, self.item_num, L.ptr_f32(W)))

    # -- what the last solve did, per item column -----------------------------------------
    def _stats(self, which):
        out = np.empty(self.item_num, np.int32)
        args = [None, None, None]
        args[which] = L.ptr_i32(out)
        self._check(self._lib.tfr_slim_get_stats(self._h, *args))
        return out

    def sweeps(self):
        """int32 [item_num]: sweeps over the coordinates each column ran"""
        return self._stats(0)

    def updates(self):
        """int32 [item_num]: coordinate updates each column applied (each reads one row of ``A``)"""
        return self._stats(1)

    def converged(self):
        """bool [item_num]: the column met the stopping rule within ``max_iter`` sweeps"""
        return self._stats(2) != 0
