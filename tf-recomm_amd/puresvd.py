"""PureSVD (Cremonesi, Koren, Turrin 2010) on the device: the rank-``factors`` truncated SVD of the binary user x item matrix
``X``, scored as ``x_u V_d V_d^T`` (include/tfrecomm.h tfr_psvd_*, csrc/puresvd.hip).

The model and the algorithm, float64 throughout, ``r = factors + oversample <= 128``::

    V <- orth(V0)                                       V0 = RandomState(seed).standard_normal((item_num, r)), made here
    iterations times:  W = X V,  Z = X^T W,  V <- orth(Z)
    W = X V,  T = W^T W,  (lambda, Qe) = eig(T)         descending; each eigenvector's largest entry positive
    sigma_j = sqrt(max(lambda_j, 0)),  Q = V Qe[:, :factors] (item factors),  P = X Q (user factors)

``orth`` is CholeskyQR twice; a start block or an iterate with fewer independent columns than ``r`` (``r > rank X``) ends the
fit with an error and the model is loaded, not fitted.  The products with ``X`` are one HIP kernel that adds the listed
rows in list order, so a user's row of ``P`` is bit for bit what ``fold_in_users`` gives for that user's list.

    m = PureSVD(user_num, item_num, factors=64).fit(user_items)
    svd = m.to_svd_model(extra_users=256)               # recommend / rank_items / similar_items / evaluate_ranking / bf16
    items, scores = m.recommend_lists(svd, new_user_items, k=10)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .item_lists import ItemListModel, _pattern


def plan(user_num, item_num, factors, oversample):
    """tfr_psvd_plan as a dict: r, lanes, chunk, ahead, sweep_cap, lds_bytes, device_bytes, gram_slices (computed on the host)"""
    lib = L.load()
    i32 = [C.c_int32() for _ in range(5)]
    i64 = [C.c_int64() for _ in range(3)]
    rc = lib.tfr_psvd_plan(int(user_num), int(item_num), int(factors), int(oversample), *[C.byref(v) for v in i32 + i64])
    if rc != L.OK:
        raise L.TfrError(rc, lib.tfr_psvd_last_error().decode("utf-8", "replace"))
    names = ("r", "lanes", "chunk", "ahead", "sweep_cap", "lds_bytes", "device_bytes", "gram_slices")
    return dict(zip(names, [v.value for v in i32 + i64]))


def _p64(a):
    return None if a is None else a.ctypes.data_as(L._f64p)


class PureSVD(ItemListModel):
    _family = "psvd"

    def __init__(self, user_num, item_num, factors=64, oversample=16, iterations=8, device=0):
        self.user_num, self.item_num = int(user_num), int(item_num)
        self.factors, self.oversample, self.iterations, self.device = int(factors), int(oversample), int(iterations), int(device)
        self.r = self.factors + self.oversample
        self.fit_ms_parts = (0.0, 0.0, 0.0)             # products, orthonormalisations, eigen step with the last products
        self._lib = L.load()
        self._h = L._p()
        self._check(self._lib.tfr_psvd_create(C.byref(self._h), self.user_num, self.item_num, self.factors, self.oversample,
                                              self.device))

    def recommend(self, *args, **kwargs):
        """not served from the lists: ``to_svd_model()`` gives the model that recommends, ranks and finds neighbours"""
        raise TypeError("PureSVD serves through to_svd_model(): call recommend / rank_items on the SvdModel it returns")

    rank_items = recommend

    @property
    def fit_ms(self):
        return float(sum(self.fit_ms_parts))

    # -- data and fit ----------------------------------------------------------------
    def load(self, user_items):
        """``user_items``: scipy sparse [user_num, item_num] (its pattern is taken) or an (indptr, items) pair.  A load forgets
        the factors."""
        self._load(user_items)
        return self

    def start_block(self, seed=0):
        return np.random.RandomState(seed).standard_normal((self.item_num, self.r))

    def fit(self, user_items=None, seed=0, start=None):
        """Loads ``user_items`` if given, then fits from ``start`` [item_num, r] (default: ``start_block(seed)``)"""
        if user_items is not None:
            self.load(user_items)
        V0 = self.start_block(seed) if start is None else np.ascontiguousarray(start, np.float64)
        if V0.shape != (self.item_num, self.r):
            raise ValueError("start must be [%d, %d], got %s" % (self.item_num, self.r, V0.shape))
        ms = (C.c_float * 3)()
        try:
            self._check(self._lib.tfr_psvd_fit(self._h, _p64(V0), self.iterations, ms))
        finally:
            self.fit_ms_parts = tuple(float(v) for v in ms)
        return self

    def _get(self, what, shape):
        out = np.empty(shape, np.float64)
        self._check(self._lib.tfr_psvd_get(self._h, what, _p64(out)))
        return out

    @property
    def singular_values(self):
        return self._get(0, (self.factors,))

    @property
    def item_factors(self):
        return self._get(1, (self.item_num, self.factors))

    @property
    def user_factors(self):
        return self._get(2, (self.user_num, self.factors))

    @property
    def ritz_values(self):
        """all r eigenvalues of T = W^T W of the last fit, descending: the squares of the r Ritz singular values"""
        return self._get(3, (self.r,))

    def sweeps(self):
        """Jacobi sweeps of the last eigen step (``fit`` or ``eig``), the last, clean one included"""
        out = C.c_int32()
        self._check(self._lib.tfr_psvd_sweeps(self._h, C.byref(out)))
        return out.value

    def residuals(self):
        """``||X^T (X q_j) - sigma_j^2 q_j||_2 / sigma_0^2`` per factor, from the factors as they stand: the convergence
        diagnostic of the subspace iteration (two more products)"""
        out = np.empty(self.factors, np.float64)
        self._check(self._lib.tfr_psvd_residuals(self._h, _p64(out)))
        return out

    def set_factors(self, item_factors, singular_values):
        """Takes a fitted model's ``item_factors`` and ``singular_values`` without a refit; needs a ``load`` (``P = X Q``)"""
        Q = np.ascontiguousarray(item_factors, np.float64)
        s = np.ascontiguousarray(singular_values, np.float64)
        if Q.shape != (self.item_num, self.factors) or s.shape != (self.factors,):
            raise ValueError("need item_factors [%d, %d] and singular_values [%d]" % (self.item_num, self.factors, self.factors))
        self._check(self._lib.tfr_psvd_set_factors(self._h, _p64(Q), _p64(s)))

    # -- the stages alone ------------------------------------------------------------
    def multiply(self, block, transpose=False):
        """``X block`` ([item_num, cols] -> [user_num, cols]) or, with ``transpose``, ``X^T block``: the product kernel alone"""
        B = np.ascontiguousarray(block, np.float64)
        n_in, n_out = (self.user_num, self.item_num) if transpose else (self.item_num, self.user_num)
        if B.ndim != 2 or B.shape[0] != n_in:
            raise ValueError("block must be [%d, cols], got %s" % (n_in, B.shape))
        out = np.empty((n_out, B.shape[1]), np.float64)
        self._check(self._lib.tfr_psvd_multiply(self._h, 1 if transpose else 0, _p64(B), B.shape[1], _p64(out)))
        return out

    def product_ms(self, cols, transpose=False, reps=10):
        """device times (ms) of ``reps`` launches of the product kernel alone at ``cols`` columns"""
        ms = (C.c_float * int(reps))()
        self._check(self._lib.tfr_psvd_product_ms(self._h, 1 if transpose else 0, int(cols), int(reps), ms))
        return [float(v) for v in ms]

    def orthonormalise(self, block):
        """``orth`` alone: (V, S, R) with V the orthonormalised copy of ``block`` [n, cols], S and R [2, cols, cols] the Gram
        matrices and upper Cholesky factors of the two passes"""
        V = np.array(block, np.float64, order="C")
        n, cols = V.shape
        S, R = np.empty((2, cols, cols)), np.empty((2, cols, cols))
        self._check(self._lib.tfr_psvd_orthonormalise(self._h, n, _p64(V), cols, _p64(S), _p64(R)))
        return V, S, R

    def eig(self, T):
        """the eigen step alone: (lambda [r] descending, Qe [r, r]) of a symmetric ``T``"""
        T = np.ascontiguousarray(T, np.float64)
        r = T.shape[0]
        if T.shape != (r, r):
            raise ValueError("T must be square")
        lam, Q = np.empty(r), np.empty((r, r))
        self._check(self._lib.tfr_psvd_eig(self._h, _p64(T), r, _p64(lam), _p64(Q)))
        return lam, Q

    # -- fold-in and serving ---------------------------------------------------------
    def _fold_in(self, indptr, ids, want=True):
        n = indptr.size - 1
        out = np.empty((n, self.factors), np.float64) if want else None
        self._check(self._lib.tfr_psvd_fold_in(self._h, n, L.ptr_i64(indptr), L.ptr_i32(ids), _p64(out)))
        return out

    def fold_in_users(self, user_items):
        """``p = x Q`` for users the model does not hold: ``user_items`` is a scipy sparse [n, item_num] or an (indptr, items)
        pair.  Exact (no solve); an empty list gives zeros; the list of a resident user gives that row of ``user_factors`` bit
        for bit.  Returns [n, factors] float64."""
        return self._fold_in(*_pattern(user_items, self.item_num, "user_items"))

    def to_svd_model(self, extra_users=0, **svd_opts):
        """An ``SvdModel(user_num + extra_users, item_num, factors)`` with P and Q cast to float32, mu = 0 and zero biases: its
        score is the dot product.  The ``extra_users`` rows after the fitted ones are zero: guest rows for ``recommend_lists``."""
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
        """Top-``k`` for users known only by their lists.  ``svd``: this model's ``to_svd_model(extra_users=g)``, ``g`` > 0.  The
        lists are folded in, their rows written as float32 into ``svd``'s guest rows on the device and ``svd.recommend`` asked
        for those rows, ``g`` lists at a time; with ``exclude`` each list's own items are left out."""
        guests = svd.user_num - self.user_num
        if guests <= 0:
            raise ValueError("svd has no guest rows: make it with to_svd_model(extra_users=...)")
        if (svd.item_num, svd.dim, svd.device) != (self.item_num, self.factors, self.device):
            raise ValueError("svd is not this model's to_svd_model()")
        indptr, ids = _pattern(user_items, self.item_num, "user_items")
        n, k = indptr.size - 1, int(k)
        items = np.empty((n, k), np.int32)
        scores = np.empty((n, k), np.float32) if return_scores else None
        if n:
            self._fold_in(indptr, ids, want=False)
        users = np.arange(self.user_num, svd.user_num, dtype=np.int32)
        for lo in range(0, n, guests):
            cnt = min(guests, n - lo)
            base, _ = svd.table_devptr(L.P)
            self._check(self._lib.tfr_psvd_export_f32(self._h, 2, lo, cnt, base + 4 * self.user_num * self.factors))
            p = indptr[lo:lo + cnt + 1]
            excl = (p - p[0], ids[p[0]:p[-1]]) if exclude else None
            got = svd.recommend(users[:cnt], k, exclude=excl, return_scores=return_scores)
            if return_scores:
                items[lo:lo + cnt], scores[lo:lo + cnt] = got
            else:
                items[lo:lo + cnt] = got
        return (items, scores) if return_scores else items
