"""Offline ranking metrics over the whole catalogue.

For a user with targets ``T`` (held-out items), exclusions ``X`` (e.g. the training items) and eligible items
``E = [0, n_items) - X``, the device gives each target ``t`` its 0-based ``rank(t)``: the number of items of ``E`` with a
non-NaN score whose key beats ``t``'s (score descending, then item id ascending, as ``recommend``), or -1 when ``t`` is in
``X`` or scores NaN (unranked).  With ``n_t = |T|`` (unranked targets count as misses), ``R`` the ranked targets and
``|E| = n_items - #distinct(X)``:

- ``hits@K = #{t : 0 <= rank(t) < K}``
- ``recall@K = hits@K / n_t``;  ``precision@K = hits@K / K``;  ``hit@K = [hits@K > 0]``
- ``ndcg@K = sum_{rank(t) < K} 1 / log2(rank(t) + 2)  /  sum_{j < min(K, n_t)} 1 / log2(j + 2)``
- ``mrr = 1 / (1 + min rank)``, 0 when nothing is ranked
- ``auc`` = the fraction of pairs ``(t in R, i in E - T)`` with ``key(t) > key(i)``, a NaN-scored ``i`` counting as below
  every target: ``sum_t (|E - T| - (rank(t) - a(t))) / (|R| |E - T|)`` with ``a(t)`` the targets ranked above ``t``;
  NaN when either set is empty.  It is ``sklearn.metrics.roc_auc_score`` of the user's scores over ``E`` when no two
  scores tie.

Users without targets get NaN everywhere; the means are over the users with at least one target (``auc`` over those where
it is defined).  Everything here is float64 NumPy; only ``evaluate_ranking``'s ``rank_items`` call runs on the device.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from .engine import exclusion_csr, rated_matrix, target_csr


def ranking_metrics(ranks, indptr, n_eligible, ks=(10,), n_targets_eligible=None):
    """Per-user metrics of ``ranks`` (int, one per target of the CSR ``indptr`` [n_users + 1], as ``rank_items`` returns).
    ``n_eligible``: ``|E|`` per user (or one number for all).  ``n_targets_eligible``: ``|T ∩ E|`` per user, for the AUC's ``|E - T|``; by default
    the ranked targets (exact unless a target outside ``X`` scores NaN).  Returns a dict of float64 arrays [n_users]:
    ``n_targets``, ``n_ranked``, ``hits@K``, ``recall@K``, ``precision@K``, ``hit@K``, ``ndcg@K`` for each K of ``ks``,
    ``mrr`` and ``auc``."""
    indptr = np.asarray(indptr, np.int64).reshape(-1)
    indptr = indptr - indptr[0]
    n = indptr.size - 1
    ranks = np.asarray(ranks, np.int64).reshape(-1)[:indptr[-1]]
    nt = np.diff(indptr).astype(np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), nt)
    ranked = ranks >= 0
    n_ranked = np.bincount(row, weights=ranked, minlength=n).astype(np.int64)
    empty = nt == 0
    nan = np.full(n, np.nan)
    out = {"n_targets": nt.astype(np.float64), "n_ranked": n_ranked.astype(np.float64)}
    for K in ks:
        K = int(K)
        if K < 1:
            raise ValueError("K must be >= 1")
        top = ranked & (ranks < K)
        hits = np.bincount(row, weights=top, minlength=n)
        dcg = np.bincount(row, weights=np.where(top, 1.0 / np.log2(np.maximum(ranks, 0) + 2.0), 0.0), minlength=n)
        ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(K, dtype=np.float64) + 2.0))])
        idcg = ideal[np.minimum(nt, K)]
        with np.errstate(invalid="ignore", divide="ignore"):
            out["hits@%d" % K] = np.where(empty, nan, hits)
            out["recall@%d" % K] = np.where(empty, nan, hits / nt)
            out["precision@%d" % K] = np.where(empty, nan, hits / K)
            out["hit@%d" % K] = np.where(empty, nan, (hits > 0).astype(np.float64))
            out["ndcg@%d" % K] = np.where(empty, nan, dcg / idcg)
    big = np.iinfo(np.int64).max
    first = np.full(n, big, np.int64)
    np.minimum.at(first, row, np.where(ranked, ranks, big))
    with np.errstate(invalid="ignore", divide="ignore"):
        out["mrr"] = np.where(empty, nan, np.where(first < big, 1.0 / (1.0 + first.astype(np.float64)), 0.0))
    # AUC: a(t) = the target's place among its row's ranked targets (ranks are distinct within a row)
    sel = np.flatnonzero(ranked)
    o = sel[np.lexsort((ranks[sel], row[sel]))]
    starts = np.concatenate([[0], np.cumsum(n_ranked)])[:-1]
    above = np.arange(o.size, dtype=np.int64) - starts[row[o]]
    te = n_ranked if n_targets_eligible is None else np.asarray(n_targets_eligible, np.int64).reshape(-1)
    neg = np.broadcast_to(np.asarray(n_eligible, np.int64), (n,)) - te
    good = np.bincount(row[o], weights=(neg[row[o]] - (ranks[o] - above)).astype(np.float64), minlength=n)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["auc"] = np.where((n_ranked > 0) & (neg > 0), good / (n_ranked * neg.astype(np.float64)), np.nan)
    return out


def _means(m):
    has = m["n_targets"] > 0
    res = {}
    for k, v in m.items():
        if k in ("n_targets", "n_ranked"):
            continue
        w = v[has]
        w = w[~np.isnan(w)]
        res[k] = float(w.mean()) if w.size else float("nan")
    return res


def evaluate_ranking(model, test_users, test_items, exclude=None, ks=(10, 20), users=None, item_lo=None, item_hi=None,
                     bf16=False):
    """Rank each user's held-out items (the ``test_users`` / ``test_items`` columns, e.g. a ``dataio`` frame's) over the whole
    catalogue on the device and report the module's metrics.  ``exclude``: as in ``recommend`` (typically
    ``rated_matrix`` of the training columns).  ``users``: the users to evaluate (default: every user with a held-out item).
    ``model``: an ``SvdModel``, or an ``FmModel`` with ``item_lo`` / ``item_hi`` (ids relative to ``item_lo``, users are
    user features).  Returns a dict: ``users``, ``indptr`` / ``items`` / ``ranks`` (the target CSR and its ranks), the
    per-user arrays of ``ranking_metrics`` and ``mean`` (each metric's mean over the users with at least one target).
    ``bf16=True`` ranks from an ``SvdModel``'s bf16 snapshot (``rank_items_bf16``, after ``snapshot_bf16``): what a service
    that answers with ``recommend_bf16`` would be measured by.  An FM model has no snapshot: ValueError."""
    fm = item_lo is not None or item_hi is not None
    if bf16 and (fm or not hasattr(model, "rank_items_bf16")):
        raise ValueError("bf16=True needs an SvdModel: only it has a bf16 snapshot")
    if fm:
        if item_lo is None or item_hi is None:
            raise ValueError("an FM model needs item_lo and item_hi")
        n_items, n_rows = int(item_hi) - int(item_lo), int(model.n_features)
    else:
        n_items, n_rows = int(model.item_num), int(model.user_num)
    T = rated_matrix(test_users, test_items, n_rows, n_items)
    if users is None:
        users = np.flatnonzero(np.diff(T.indptr)).astype(np.int32)
    users = L.as_i32(users, "user ids").reshape(-1)
    if users.size and (users.min() < 0 or users.max() >= n_rows):
        raise L.OutOfRangeError(L.ERR_OOB, "users outside [0, %d)" % n_rows)
    indptr, items, _ = target_csr(T, users)
    xp, xi = exclusion_csr(exclude, users)
    ex = None if xp is None else (xp, xi)
    if fm:
        ranks = model.rank_items(users, item_lo, item_hi, (indptr, items), exclude=ex)
    else:
        ranks = (model.rank_items_bf16 if bf16 else model.rank_items)(users, (indptr, items), exclude=ex)
    n = users.size
    n_elig = np.full(n, n_items, np.int64)
    t_elig = np.diff(indptr).astype(np.int64)
    if xp is not None:
        xi = np.asarray(xi[xp[0]:xp[-1]], np.int64)
        xp = xp - xp[0]
        xrow = np.repeat(np.arange(n, dtype=np.int64), np.diff(xp))
        first = np.ones(xi.size, bool)
        first[1:] = (xi[1:] != xi[:-1]) | (xrow[1:] != xrow[:-1])
        n_elig -= np.bincount(xrow[first], minlength=n)
        trow = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
        inx = np.isin(trow * n_items + items, xrow * n_items + xi)
        t_elig -= np.bincount(trow[inx], minlength=n)
    m = ranking_metrics(ranks, indptr, n_elig, ks, n_targets_eligible=t_elig)
    res = dict(users=users, indptr=indptr, items=items, ranks=ranks)
    res.update(m)
    res["mean"] = _means(m)
    return res
