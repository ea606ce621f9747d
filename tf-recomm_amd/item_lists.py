"""What ``ItemKNN``, ``EASE`` and ``SLIM`` share: each holds a binary user x item CSR on the device and serves from it through C
entries that differ only in their family prefix (csrc/item_lists.h is the native side of this module)."""
from __future__ import annotations

import numpy as np

from . import _lib as L
from .engine import exclusion_csr, rank_call


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


class ItemListModel(object):
    """The handle and the serving calls of a family whose C symbols are ``tfr_<_family>_*``.  A subclass sets ``_family``,
    ``user_num`` and ``item_num``, and its constructor loads ``_lib`` and creates ``_h``."""
    _family = None

    def _c(self, name):
        return getattr(self._lib, "tfr_%s_%s" % (self._family, name))

    def _check(self, rc):
        if rc != L.OK:
            text = self._c("last_error")().decode("utf-8", "replace")
            raise (L.OutOfRangeError if rc == L.ERR_OOB else L.TfrError)(rc, text)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._c("destroy")(self._h)
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

    def _load(self, user_items):
        indptr, items = _pattern(user_items, self.item_num, "user_items")
        if indptr.size != self.user_num + 1:
            raise ValueError("user_items must hold %d rows" % self.user_num)
        self._check(self._c("load")(self._h, L.ptr_i64(indptr), L.ptr_i32(items)))

    # -- serving ------------------------------------------------------------------------
    def recommend(self, users, k=10, exclude=None, return_scores=True):
        """The ``k`` best items of each of ``users`` (resident: their loaded rows are the lists), best first, equal scores by
        item id.  ``exclude`` as in ``SvdModel.recommend``.  Returns ``items`` int32 [n, k] (-1 past the eligible items) and,
        if asked, ``scores`` float32 [n, k] (-inf there)."""
        u = L.as_i32(users, "user ids").reshape(-1)
        xp, xi = exclusion_csr(exclude, u)
        items = np.empty((u.size, int(k)), np.int32)
        scores = np.empty((u.size, int(k)), np.float32) if return_scores else None
        self._check(self._c("topk")(self._h, L.ptr_i32(u), u.size, int(k), None if xp is None else L.ptr_i64(xp),
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
        self._check(self._c("topk_lists")(self._h, L.ptr_i64(indptr), L.ptr_i32(ids), n, int(k),
                                          None if xp is None else L.ptr_i64(xp), None if xi is None else L.ptr_i32(xi),
                                          L.ptr_i32(items), None if scores is None else L.ptr_f32(scores)))
        return (items, scores) if return_scores else items

    def rank_items(self, users, targets, exclude=None):
        """0-based rank of each target item of each of ``users`` among all items not in ``exclude``, by the keys of
        ``recommend``: ``rank < k`` exactly when ``recommend(users, k, exclude)`` holds the target, at that position; -1 for
        an excluded target.  Arguments and return value as ``SvdModel.rank_items``."""
        u = L.as_i32(users, "user ids").reshape(-1)

        def call(ip, it, xp, xi, out):
            self._check(self._c("rank_items")(self._h, L.ptr_i32(u), u.size, ip, it, xp, xi, out))
        return rank_call(call, u, targets, exclude)
