"""NumPy restatement of ItemKNN (include/tfrecomm.h, the tfr_knn block): what tests/test_itemknn_host.py checks by hand and
tests/test_gpu_itemknn.py holds the device to, bit for bit.

Counts are int64 from ``X.T @ X``; similarities are float64 NumPy expressions rounded once by ``astype(float32)``; user scores
are a Python loop of float32 adds in list order; top-K and ranks come from the ``tfr_topk`` key over all non-excluded items."""
import numpy as np
import scipy.sparse as sp


def pattern(indptr, items, n_users, n_items):
    indptr = np.asarray(indptr, np.int64)
    items = np.asarray(items, np.int64)
    return sp.csr_matrix((np.ones(items.size, np.int64), items, indptr), shape=(n_users, n_items))


def cooccurrence(indptr, items, n_users, n_items):
    """(C int64 CSR with sorted rows, n int64 [n_items]): C = X^T X, n = its diagonal = users per item"""
    x = pattern(indptr, items, n_users, n_items)
    c = (x.T @ x).tocsr().astype(np.int64)
    c.sort_indices()
    n = np.asarray(x.sum(axis=0)).reshape(-1).astype(np.int64)
    return c, n


def similarity(c, ni, nj, metric, shrink):
    """float32 similarities of integer arrays c, ni, nj"""
    c = np.asarray(c, np.int64)
    ni = np.asarray(ni, np.int64)
    nj = np.asarray(nj, np.int64)
    cd = c.astype(np.float64)
    if metric == "cosine":
        s = cd / (np.sqrt(ni.astype(np.float64) * nj.astype(np.float64)) + np.float64(shrink))
    elif metric == "jaccard":
        s = cd / ((ni + nj - c).astype(np.float64) + np.float64(shrink))
    elif metric == "count":
        assert shrink == 0
        s = cd
    else:
        raise ValueError(metric)
    return s.astype(np.float32)


def fit(c, n, K, metric, shrink):
    """neighbour lists (items int32 [I, K], scores float32 [I, K]) from cooccurrence()'s output: per row the K best of
    c > 0, j != i by (-score, id), padded with -1 / -inf"""
    n_items = n.size
    nb = np.full((n_items, K), -1, np.int32)
    sc = np.full((n_items, K), -np.inf, np.float32)
    for i in range(n_items):
        lo, hi = c.indptr[i], c.indptr[i + 1]
        js, cs = c.indices[lo:hi].astype(np.int64), c.data[lo:hi]
        keep = (cs > 0) & (js != i)
        js, cs = js[keep], cs[keep]
        if js.size == 0:
            continue
        s = similarity(cs, np.full(js.size, n[i]), n[js], metric, shrink)
        order = np.lexsort((js, -s))[:K]
        nb[i, :order.size] = js[order]
        sc[i, :order.size] = s[order]
    return nb, sc


def user_scores(lst, nb, sc, n_items):
    """float32 [n_items]: for i in the list, in the order given (ascending), acc[nb[i]] += sc[i], skipping -1"""
    acc = np.zeros(n_items, np.float32)
    for i in lst:
        row = nb[i]
        m = row >= 0
        acc[row[m]] = acc[row[m]] + sc[i][m]               # one item's neighbours are distinct columns
    return acc


def keys(scores):
    """the tfr_topk key of every item of a float32 score vector: ordered uint32 of the score << 32 | ~item"""
    b = np.asarray(scores, np.float32).view(np.uint32).astype(np.uint64)
    o = np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xffffffff), b | np.uint64(0x80000000))
    ids = np.arange(b.size, dtype=np.uint64)
    return (o << np.uint64(32)) | (~ids & np.uint64(0xffffffff))


def topk(scores, k, excl=()):
    """(items int32 [k], scores float32 [k]) over the items outside excl, key descending, padded with -1 / -inf"""
    key = keys(scores)
    ok = ~np.isnan(scores)
    ok[np.asarray(excl, np.int64)] = False
    cand = np.flatnonzero(ok)
    best = cand[np.argsort(key[cand])[::-1][:k]]
    items = np.full(k, -1, np.int32)
    out = np.full(k, -np.inf, np.float32)
    items[:best.size] = best
    out[:best.size] = scores[best]
    return items, out


def ranks(scores, targets, excl=()):
    """int32 rank of each target: eligible items whose key is above the target's; -1 for an excluded target"""
    key = keys(scores)
    ok = ~np.isnan(scores)
    ok[np.asarray(excl, np.int64)] = False
    elig = np.sort(key[ok])
    out = np.empty(len(targets), np.int32)
    for z, t in enumerate(targets):
        out[z] = elig.size - np.searchsorted(elig, key[t], side="right") if ok[t] else -1
    return out
