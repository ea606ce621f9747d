"""NumPy statement of the ranking contract (include/tfrecomm.h tfr_rank_items) and of the metrics of
tfrecomm_amd.ranking, by brute force over the full score row."""
import math

import numpy as np

from tests.topk_ref import ordered_u32


def keys(S_row):
    """the 64-bit key of every item of one float32 score row: order-preserving uint32 of the score, then ~item"""
    I = S_row.size
    return (ordered_u32(S_row).astype(np.uint64) << np.uint64(32)) | (~np.arange(I, dtype=np.uint64) & np.uint64(0xffffffff))


def rank_ref(S, targets, excl=None):
    """S float32 [n, I]; targets: n arrays of items; excl None or n arrays.  Returns the ranks concatenated row by row."""
    S = np.asarray(S, np.float32)
    out = []
    for r in range(S.shape[0]):
        k = keys(S[r])
        ok = ~np.isnan(S[r])
        if excl is not None and len(excl[r]):
            ok[np.asarray(excl[r], np.int64)] = False
        kk = k[ok]
        for t in np.asarray(targets[r], np.int64):
            out.append(int(np.count_nonzero(kk > k[t])) if ok[t] else -1)
    return np.asarray(out, np.int64)


def metrics_brute(S_row, T, X, ks):
    """One user's metrics straight from the definitions (pairs and positions over the whole row)."""
    S_row = np.asarray(S_row, np.float32)
    I = S_row.size
    k = keys(S_row)
    nan = np.isnan(S_row)
    E = np.ones(I, bool)
    if len(X):
        E[np.asarray(X, np.int64)] = False
    T = [int(t) for t in T]
    n_t = len(T)
    ranks = {}
    for t in T:
        ranks[t] = int(np.count_nonzero(E & ~nan & (k > k[t]))) if E[t] and not nan[t] else -1
    res = {}
    if n_t == 0:
        for K in ks:
            for m in ("hits", "recall", "precision", "hit", "ndcg"):
                res["%s@%d" % (m, K)] = float("nan")
        res["mrr"] = res["auc"] = float("nan")
        return res, ranks
    for K in ks:
        hits = sum(1 for t in T if 0 <= ranks[t] < K)
        res["hits@%d" % K] = float(hits)
        res["recall@%d" % K] = hits / n_t
        res["precision@%d" % K] = hits / K
        res["hit@%d" % K] = float(hits > 0)
        dcg = sum(1.0 / math.log2(ranks[t] + 2) for t in T if 0 <= ranks[t] < K)
        idcg = sum(1.0 / math.log2(j + 2) for j in range(min(K, n_t)))
        res["ndcg@%d" % K] = dcg / idcg
    rk = [ranks[t] for t in T if ranks[t] >= 0]
    res["mrr"] = 1.0 / (1 + min(rk)) if rk else 0.0
    R = [t for t in T if ranks[t] >= 0]
    Tset = set(T)
    neg = [i for i in range(I) if E[i] and i not in Tset]
    if not R or not neg:
        res["auc"] = float("nan")
    else:
        good = sum(1 for t in R for i in neg if nan[i] or k[t] > k[i])
        res["auc"] = good / (len(R) * len(neg))
    return res, ranks
