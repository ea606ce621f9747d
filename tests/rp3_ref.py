"""NumPy restatement of the weighted co-occurrence fit and of RP3beta on it (include/tfrecomm.h, tfr_knn_fit_weighted): what
tests/test_rp3_host.py checks by hand and tests/test_gpu_rp3.py holds the device to, bit for bit.

``S = X^T diag(q) X`` is an int64 sparse product (exact: the callers keep every sum below 2^63); the similarity is the float64
chain ``S.astype(float64) * 2^-shift * row_scale[i] * col_scale[j]``, left to right, then ``.astype(float32)``; the lists are
``lexsort`` by (-score, id) over ``S > 0, j != i``.  User scores, top-K and ranks on the lists are tests/itemknn_ref.py's."""
import numpy as np
import scipy.sparse as sp

from tests import itemknn_ref as R


def weighted_sums(indptr, items, n_users, n_items, q):
    """S int64 CSR with sorted rows, explicit zeros dropped: S_ij = sum of q[u] over the users with both i and j"""
    q = np.asarray(q, np.uint64)
    assert q.shape == (n_users,) and (q.size == 0 or int(q.max()) < 2 ** 63)
    x = R.pattern(indptr, items, n_users, n_items)
    xq = x.copy()                                          # diag(q) X with int64 values: nothing passes through float64
    xq.data = np.repeat(q.astype(np.int64), np.diff(x.indptr))
    s = (x.T @ xq).tocsr()
    assert s.dtype == np.int64
    s.eliminate_zeros()
    s.sort_indices()
    return s


def fit(s, row_scale, col_scale, shift, K):
    """neighbour lists (items int32 [I, K], scores float32 [I, K]) from weighted_sums()' output"""
    row_scale = np.asarray(row_scale, np.float64)
    col_scale = np.asarray(col_scale, np.float64)
    n_items = row_scale.size
    unit = np.float64(2.0) ** -int(shift)
    nb = np.full((n_items, K), -1, np.int32)
    sc = np.full((n_items, K), -np.inf, np.float32)
    for i in range(n_items):
        lo, hi = s.indptr[i], s.indptr[i + 1]
        js, ss = s.indices[lo:hi].astype(np.int64), s.data[lo:hi]
        keep = (ss > 0) & (js != i)
        js, ss = js[keep], ss[keep]
        if js.size == 0:
            continue
        v = (((ss.astype(np.float64) * unit) * row_scale[i]) * col_scale[js]).astype(np.float32)
        order = np.lexsort((js, -v))[:K]
        nb[i, :order.size] = js[order]
        sc[i, :order.size] = v[order]
    return nb, sc


def shift_for(max_item_users):
    return min(40, 62 - int(max_item_users).bit_length())


def neg_power(counts, exponent):
    n = np.asarray(counts, np.float64)
    return np.where(n > 0, np.power(np.where(n > 0, n, 1.0), -np.float64(exponent)), 0.0)


def rp3_terms(indptr, items, n_users, n_items, alpha, beta, shift=None):
    """(q uint64 [n_users], row_scale, col_scale float64 [n_items], shift) of RP3beta, in NumPy float64"""
    deg = np.diff(np.asarray(indptr, np.int64))
    n = np.bincount(np.asarray(items, np.int64), minlength=n_items)
    shift = shift_for(n.max() if n.size else 0) if shift is None else shift
    w = neg_power(deg, alpha)
    q = np.rint(w * np.float64(2.0) ** shift).astype(np.uint64)
    return q, neg_power(n, alpha), neg_power(n, beta), shift


def rp3_fit(indptr, items, n_users, n_items, K, alpha, beta):
    q, rs, cs, shift = rp3_terms(indptr, items, n_users, n_items, alpha, beta)
    return fit(weighted_sums(indptr, items, n_users, n_items, q), rs, cs, shift, K)


def rp3_float64(indptr, items, n_users, n_items, alpha, beta):
    """the unrounded model: diag(n^-alpha) X^T diag(d^-alpha) X diag(n^-beta) as a float64 CSR"""
    x = R.pattern(indptr, items, n_users, n_items).astype(np.float64)
    deg = np.diff(np.asarray(indptr, np.int64))
    n = np.bincount(np.asarray(items, np.int64), minlength=n_items)
    m = sp.diags(neg_power(n, alpha)) @ x.T @ sp.diags(neg_power(deg, alpha)) @ x @ sp.diags(neg_power(n, beta))
    return m.tocsr()
