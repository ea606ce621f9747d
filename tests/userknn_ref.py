"""NumPy restatement of UserKNN (include/tfrecomm.h, the tfr_uknn block): what tests/test_userknn_host.py checks by hand and
tests/test_gpu_userknn.py holds the device to, bit for bit.

Counts are int64 from ``X @ X.T``; similarities, keys, top-K and ranks are tests/itemknn_ref.py's; user scores are a Python
loop of float32 adds over the neighbour slots in list order."""
import numpy as np

from tests import itemknn_ref as IR

similarity, keys, topk, ranks = IR.similarity, IR.keys, IR.topk, IR.ranks


def cooccurrence(indptr, items, n_users, n_items):
    """(C int64 CSR with sorted rows [n_users, n_users], d int64 [n_users]): C = X X^T, d = its diagonal = items per user"""
    x = IR.pattern(indptr, items, n_users, n_items)
    c = (x @ x.T).tocsr().astype(np.int64)
    c.sort_indices()
    return c, np.diff(np.asarray(indptr, np.int64))


def fit(indptr, items, nu, ni, K, metric, shrink):
    """neighbour lists (users int32 [nu, K], scores float32 [nu, K]): per user the K best of c > 0, v != u by (-score, id),
    padded with -1 / -inf"""
    c, d = cooccurrence(indptr, items, nu, ni)
    nb = np.full((nu, K), -1, np.int32)
    sc = np.full((nu, K), -np.inf, np.float32)
    for u in range(nu):
        lo, hi = c.indptr[u], c.indptr[u + 1]
        vs, cs = c.indices[lo:hi].astype(np.int64), c.data[lo:hi]
        keep = (cs > 0) & (vs != u)
        vs, cs = vs[keep], cs[keep]
        if vs.size == 0:
            continue
        s = similarity(cs, np.full(vs.size, d[u]), d[vs], metric, shrink)
        order = np.lexsort((vs, -s))[:K]
        nb[u, :order.size] = vs[order]
        sc[u, :order.size] = s[order]
    return nb, sc


def list_neighbours(lst, indptr, items, nu, ni, K, metric, shrink):
    """(users int32 [K], scores float32 [K]) of a user known only by its list: the K best resident users sharing an item,
    similarity from (|L n N(v)|, |L|, d_v); nobody is left out as self"""
    lst = np.asarray(lst, np.int64)
    x = IR.pattern(indptr, items, nu, ni)
    mark = np.zeros(ni, np.int64)
    mark[lst] = 1
    c = np.asarray(x @ mark).reshape(-1)
    d = np.diff(np.asarray(indptr, np.int64))
    vs = np.flatnonzero(c > 0)
    nb = np.full(K, -1, np.int32)
    sc = np.full(K, -np.inf, np.float32)
    if vs.size:
        s = similarity(c[vs], np.full(vs.size, lst.size), d[vs], metric, shrink)
        order = np.lexsort((vs, -s))[:K]
        nb[:order.size] = vs[order]
        sc[:order.size] = s[order]
    return nb, sc


def user_scores(nb_row, sc_row, indptr, items, ni):
    """float32 [ni]: for each slot in order, slot 0 first, acc[N(v)] += s, skipping -1"""
    acc = np.zeros(ni, np.float32)
    for v, s in zip(nb_row, sc_row):
        if v < 0:
            continue
        row = items[indptr[v]:indptr[v + 1]]
        acc[row] = acc[row] + np.float32(s)                # one neighbour's items are distinct columns
    return acc
