"""RP3beta timings (tfr_knn_fit_weighted against tfr_knn_fit): one JSON object per measurement, on ML-1M-shaped synthetic pairs
(6040 users x 3706 items, about 1 M distinct pairs, items drawn from a Zipf law, users uniform), K = 100 and K = 20.

``fit``: the device times the two fits report (events around their launches; the weighted fit's upload of the weights and
scales comes before its first event), alternating fit by fit on two handles in one process, median and best of ``--reps``
after 3 warm-ups each, and their ratio: the cost of 64-bit against 32-bit LDS atomics plus one more load per user.  Beside
them the host's way to the same model: scipy ``diag(n^-alpha) X^T diag(d^-alpha) X diag(n^-beta)`` and a per-row
``argpartition`` of the K best (wall clock, median of 3, at most 16 threads).
``recommend``: every user, k = 10, each user's own items excluded, through the host entry (wall clock around the call).
These are records; no ratio is a gate.
python tools/bench_rp3beta.py [--reps N] [--out profiles/bench_rp3beta.jsonl]"""
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

U, I, PAIRS = 6040, 3706, 1_000_000
ALPHA, BETA = 1.0, 0.6


def synthetic(seed=0):
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(I) + 10.0)
    p /= p.sum()
    n = int(PAIRS * 1.35)                                  # repeats of popular items are merged: aim past the target
    x = sp.csr_matrix((np.ones(n, np.float32), (rng.integers(0, U, n), rng.choice(I, n, p=p))), shape=(U, I))
    x.sum_duplicates()
    x.data[:] = 1.0
    return x


def host_fit(x, K):
    x = x.astype(np.float64)
    d = np.asarray(x.sum(axis=1)).reshape(-1)
    n = np.asarray(x.sum(axis=0)).reshape(-1)
    inv = lambda v, e: np.where(v > 0, np.power(np.maximum(v, 1.0), -e), 0.0)
    w = (sp.diags(inv(n, ALPHA)) @ x.T @ sp.diags(inv(d, ALPHA)) @ x @ sp.diags(inv(n, BETA))).tocsr()
    nb = np.full((I, K), -1, np.int32)
    for i in range(I):
        lo, hi = w.indptr[i], w.indptr[i + 1]
        js, s = w.indices[lo:hi], w.data[lo:hi]
        keep = js != i
        js, s = js[keep], s[keep]
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
    lines = []

    def emit(**rec):
        lines.append(json.dumps(dict(dict(users=U, items=I, pairs=int(x.nnz)), **rec)))
        print(lines[-1], flush=True)

    users = np.arange(U, dtype=np.int32)
    for K in (100, 20):
        host = wall(lambda: host_fit(x, K), 3, warmup=1)
        with T.RP3beta(U, I, K=K, alpha=ALPHA, beta=BETA) as rp3, T.ItemKNN(U, I, K=K, metric="count") as knn:
            rp3.fit(x)
            knn.load(x)
            q, shift = rp3.q, rp3.shift
            n = np.asarray(x.sum(axis=0)).reshape(-1)
            rs, cs = np.where(n > 0, np.maximum(n, 1.0) ** -ALPHA, 0.0), np.where(n > 0, np.maximum(n, 1.0) ** -BETA, 0.0)
            arms = {"weighted": lambda: rp3.fit_raw(q, rs, cs, shift), "count": lambda: knn.fit()}
            models = {"weighted": rp3, "count": knn}
            ms = {name: [] for name in arms}
            for r in range(3 + a.reps):
                for name, fn in arms.items():
                    fn()
                    if r >= 3:
                        ms[name].append(models[name].fit_ms)
            med = {name: float(np.median(v)) for name, v in ms.items()}
            emit(what="fit", K=K, alpha=ALPHA, beta=BETA, shift=shift, reps=a.reps,
                 weighted_fit_ms_median=round(med["weighted"], 3), weighted_fit_ms_min=round(float(np.min(ms["weighted"])), 3),
                 count_fit_ms_median=round(med["count"], 3), count_fit_ms_min=round(float(np.min(ms["count"])), 3),
                 weighted_over_count=round(med["weighted"] / med["count"], 3),
                 host_scipy_ms_median=round(float(np.median(host)), 1), host_over_device=round(float(np.median(host)) / med["weighted"], 1))
            ts = wall(lambda: rp3.recommend(users, 10, exclude=x), a.reps)
            emit(what="recommend", K=K, k=10, queries=U, exclusions="own items", reps=a.reps,
                 rp3beta_ms_median=round(float(np.median(ts)), 3), rp3beta_ms_min=round(float(np.min(ts)), 3))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
