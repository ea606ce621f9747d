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

    # -- serving --------------------------------------------------------------------
    def to_svd_model(self, **svd_opts):
        """An ``SvdModel(user_num, item_num, factors)`` with P = X and Q = Y cast to float32, mu = 0 and zero biases: its
        score is the dot product.  Copies through the host."""
        from .engine import SvdModel
        svd_opts.setdefault("device", self.device)
        m = SvdModel(self.user_num, self.item_num, self.factors, **svd_opts)
        m.set_tables(np.float32(0.0), np.zeros(self.user_num, np.float32), np.zeros(self.item_num, np.float32),
                     self.user_factors.astype(np.float32), self.item_factors.astype(np.float32))
        return m
