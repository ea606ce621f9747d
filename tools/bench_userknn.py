"""UserKNN timings (tfr_uknn_fit, tfr_uknn_topk, tfr_uknn_topk_lists): one JSON object per measurement, on the ML-1M-shaped
synthetic pairs of tools/bench_itemknn.py (6040 users x 3706 items, about 1.08 M distinct pairs, items drawn from a Zipf
law, users uniform), K = 50.

``fit``: the device time tfr_uknn_fit reports (events around its launches), median and best of ``--reps`` fits after 3
warm-up fits, per metric; beside it the host's way to the same lists: scipy ``X @ X.T`` and a per-row ``argpartition`` of
the K best (wall clock, median of 3, at most 16 threads).
``recommend``: every user, k = 10, each user's own items excluded, through the host entry (wall clock around the call: upload
of the ids and the exclusion CSR, launches, download), alternating call by call with ``ItemKNN.recommend`` (K = 20) on the
same matrix in the same process; medians and minima of ``--reps`` calls after 3 warm-up calls each.
``recommend_lists``: the same users given as lists to a handle that was only loaded: the neighbour search and the scoring.
These are records; no ratio is a gate.
python tools/bench_userknn.py [--reps N] [--out profiles/bench_userknn.jsonl]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tfrecomm_amd as T
from tools.bench_itemknn import I, U, synthetic, wall

K, K_ITEM = 50, 20


def host_fit(x):
    c = (x @ x.T).tocsr()
    d = np.asarray(x.sum(axis=1)).reshape(-1)
    nb = np.full((U, K), -1, np.int32)
    for u in range(U):
        lo, hi = c.indptr[u], c.indptr[u + 1]
        vs, cs = c.indices[lo:hi], c.data[lo:hi]
        keep = vs != u
        vs, cs = vs[keep], cs[keep]
        s = cs / np.sqrt(d[u] * d[vs])
        if s.size > K:
            top = np.argpartition(-s, K - 1)[:K]
            vs, s = vs[top], s[top]
        nb[u, :vs.size] = vs[np.argsort(-s, kind="stable")]
    return nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.init()
    x = synthetic()
    shape = dict(users=U, items=I, pairs=int(x.nnz), K=K)
    lines = []

    def emit(**rec):
        lines.append(json.dumps(dict(shape, **rec)))
        print(lines[-1], flush=True)

    host = wall(lambda: host_fit(x), 3, warmup=1)
    for metric in ("cosine", "jaccard", "count"):
        with T.UserKNN(U, I, K=K, metric=metric) as m:
            m.load(x)
            ms = []
            for r in range(3 + a.reps):
                m.fit()
                if r >= 3:
                    ms.append(m.fit_ms)
            rec = dict(what="fit", metric=metric, reps=a.reps, fit_ms_median=round(float(np.median(ms)), 3),
                       fit_ms_min=round(float(np.min(ms)), 3))
            if metric == "cosine":
                rec.update(host_scipy_ms_median=round(float(np.median(host)), 1),
                           host_over_device=round(float(np.median(host) / np.median(ms)), 1))
            emit(**rec)

    users = np.arange(U, dtype=np.int32)
    with T.UserKNN(U, I, K=K) as m, T.UserKNN(U, I, K=K) as loaded, T.ItemKNN(U, I, K=K_ITEM) as item:
        m.fit(x)
        loaded.load(x)
        item.fit(x)
        arms = {"userknn": lambda: m.recommend(users, 10, exclude=x), "itemknn": lambda: item.recommend(users, 10, exclude=x),
                "userknn_lists": lambda: loaded.recommend_lists(x, 10)}
        for fn in arms.values():
            for _ in range(3):
                fn()
        ts = {name: [] for name in arms}
        for _ in range(a.reps):
            for name, fn in arms.items():
                t = time.perf_counter()
                fn()
                ts[name].append((time.perf_counter() - t) * 1e3)
        med = {name: float(np.median(v)) for name, v in ts.items()}
        emit(what="recommend", k=10, queries=U, exclusions="own items", reps=a.reps, itemknn_K=K_ITEM,
             userknn_ms_median=round(med["userknn"], 3), userknn_ms_min=round(float(np.min(ts["userknn"])), 3),
             itemknn_ms_median=round(med["itemknn"], 3), itemknn_ms_min=round(float(np.min(ts["itemknn"])), 3),
             userknn_over_itemknn=round(med["userknn"] / med["itemknn"], 3))
        emit(what="recommend_lists", k=10, queries=U, exclusions="own items", reps=a.reps,
             userknn_lists_ms_median=round(med["userknn_lists"], 3), userknn_lists_ms_min=round(float(np.min(ts["userknn_lists"])), 3),
             lists_over_resident=round(med["userknn_lists"] / med["userknn"], 3))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
