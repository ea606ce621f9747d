"""ItemKNN timings (tfr_knn_fit, tfr_knn_topk): one JSON object per measurement, on ML-1M-shaped synthetic pairs
(6040 users x 3706 items, about 1 M distinct pairs, items drawn from a Zipf law, users uniform), K = 20.

``fit``: the device time tfr_knn_fit reports (events around its launches), median and best of ``--reps`` fits after 3
warm-up fits, per metric; beside it the host's way to the same lists: scipy ``X.T @ X`` and a per-row ``argpartition`` of
the K best (wall clock, median of 3, at most 16 threads).
``recommend``: every user, k = 10, each user's own items excluded, through the host entry (wall clock around the call: upload
of the ids and the exclusion CSR, launches, download), alternating call by call with ``SvdModel.recommend`` at D = 64 on the
same shape in the same process; medians and minima of ``--reps`` calls after 3 warm-up calls each.
These are records; no ratio is a gate.
python tools/bench_itemknn.py [--reps N] [--out profiles/bench_itemknn.jsonl]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import tfrecomm_amd as T

U, I, PAIRS, K = 6040, 3706, 1_000_000, 20


def synthetic(seed=0):
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(I) + 10.0)
    p /= p.sum()
    n = int(PAIRS * 1.35)                                  # repeats of popular items are merged: aim past the target
    x = sp.csr_matrix((np.ones(n, np.float32), (rng.integers(0, U, n), rng.choice(I, n, p=p))), shape=(U, I))
    x.sum_duplicates()
    x.data[:] = 1.0
    return x


def host_fit(x, metric="cosine"):
    c = (x.T @ x).tocsr()
    n = np.asarray(x.sum(axis=0)).reshape(-1)
    nb = np.full((I, K), -1, np.int32)
    for i in range(I):
        lo, hi = c.indptr[i], c.indptr[i + 1]
        js, cs = c.indices[lo:hi], c.data[lo:hi]
        keep = js != i
        js, cs = js[keep], cs[keep]
        s = cs / np.sqrt(n[i] * n[js])
        if s.size > K:
            top = np.argpartition(-s, K - 1)[:K]
            js, s = js[top], s[top]
        nb[i, :js.size] = js[np.argsort(-s, kind="stable")]
    return nb


def wall(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


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
        with T.ItemKNN(U, I, K=K, metric=metric) as m:
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

    rng = np.random.default_rng(1)
    users = np.arange(U, dtype=np.int32)
    with T.ItemKNN(U, I, K=K) as m, T.SvdModel(U, I, 64) as svd:
        m.fit(x)
        svd.set_tables(np.float32(0.1), rng.standard_normal(U, dtype=np.float32) * .5, rng.standard_normal(I, dtype=np.float32) * .5,
                       rng.standard_normal((U, 64), dtype=np.float32) * .3, rng.standard_normal((I, 64), dtype=np.float32) * .3)
        arms = {"itemknn": lambda: m.recommend(users, 10, exclude=x), "svd_d64": lambda: svd.recommend(users, 10, exclude=x)}
        for fn in arms.values():
            for _ in range(3):
                fn()
        ts = {name: [] for name in arms}
        for _ in range(a.reps):
            for name, fn in arms.items():
                t = time.perf_counter()
                fn()
                ts[name].append((time.perf_counter() - t) * 1e3)
        emit(what="recommend", k=10, queries=U, exclusions="own items", reps=a.reps,
             itemknn_ms_median=round(float(np.median(ts["itemknn"])), 3), itemknn_ms_min=round(float(np.min(ts["itemknn"])), 3),
             svd_d64_ms_median=round(float(np.median(ts["svd_d64"])), 3), svd_d64_ms_min=round(float(np.min(ts["svd_d64"])), 3),
             itemknn_over_svd=round(float(np.median(ts["itemknn"]) / np.median(ts["svd_d64"])), 3))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
