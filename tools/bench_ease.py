"""EASE timings (tfr_ease_gram, tfr_ease_solve, tfr_ease_topk): one JSON object per measurement, on bench_itemknn.py's
ML-1M-shaped synthetic pairs (6040 users x 3706 items, about 1 M distinct pairs, items drawn from a Zipf law, users uniform).

``fit``: the three device times tfr_ease_solve reports (events around the launches of the Gram kernel, of the inverse and of
the weights kernel), medians and minima of ``--reps`` fits after 3 warm-up fits; beside them the wall time of NumPy's float64
``np.linalg.inv`` of the same Gram matrix on the host (median of 3, at most 16 threads).
``recommend``: every user, k = 10, each user's own items excluded, through the host entry (wall clock around the call),
alternating call by call with ``ItemKNN.recommend`` (K = 20, cosine) in the same process; medians and minima of ``--reps``
calls after 3 warm-up calls each.
``inverse``: one larger catalogue, 16384 items (the same law, 4 M draws), the inverse alone: median of 3 after 1 warm-up, and
the float64 rate n^3 / time - the useful operations of the three sweeps (n^3 / 3 each), not those the tiles execute.
These are records; no ratio is a gate.
python tools/bench_ease.py [--reps N] [--skip-large] [--out profiles/bench_ease.jsonl]"""
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
from tools.bench_itemknn import synthetic, wall, U, I

LAMBDA = 500.0
BIG_I, BIG_DRAWS = 16384, 4_000_000


def synthetic_big(seed=2):
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(BIG_I) + 10.0)
    p /= p.sum()
    x = sp.csr_matrix((np.ones(BIG_DRAWS, np.float32), (rng.integers(0, U, BIG_DRAWS), rng.choice(BIG_I, BIG_DRAWS, p=p))),
                      shape=(U, BIG_I))
    x.sum_duplicates()
    x.data[:] = 1.0
    return x


def med(v):
    return round(float(np.median(v)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.init()
    x = synthetic()
    shape = dict(users=U, items=I, pairs=int(x.nnz), regularization=LAMBDA)
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    users = np.arange(U, dtype=np.int32)
    with T.EASE(U, I, regularization=LAMBDA) as m, T.ItemKNN(U, I, K=20) as knn:
        m.load(x)
        g = m.gram()
        host = wall(lambda: np.linalg.inv(g), 3, warmup=1)
        parts = {"gram": [], "inverse": [], "weights": []}
        for r in range(3 + a.reps):
            m.fit()
            if r >= 3:
                for name in parts:
                    parts[name].append(m.fit_ms_parts[name])
        total = np.sum([parts[name] for name in parts], axis=0)
        plan = T.ease.plan(I)
        emit(**dict(shape, what="fit", reps=a.reps, nb=plan["nb"], tile=plan["tile"], fit_ms_median=med(total),
                    fit_ms_min=round(float(total.min()), 3), gram_ms_median=med(parts["gram"]),
                    inverse_ms_median=med(parts["inverse"]), inverse_ms_min=round(float(np.min(parts["inverse"])), 3),
                    weights_ms_median=med(parts["weights"]), host_numpy_inv_ms_median=round(float(np.median(host)), 1),
                    host_inv_over_device_inverse=round(float(np.median(host) / np.median(parts["inverse"])), 2),
                    inverse_f64_tflops=round(float(I) ** 3 / (np.median(parts["inverse"]) * 1e-3) / 1e12, 3)))

        knn.fit(x)
        arms = {"ease": lambda: m.recommend(users, 10, exclude=x), "itemknn": lambda: knn.recommend(users, 10, exclude=x)}
        for fn in arms.values():
            for _ in range(3):
                fn()
        ts = {name: [] for name in arms}
        for _ in range(a.reps):
            for name, fn in arms.items():
                t = time.perf_counter()
                fn()
                ts[name].append((time.perf_counter() - t) * 1e3)
        emit(**dict(shape, what="recommend", k=10, queries=U, exclusions="own items", reps=a.reps,
                    ease_ms_median=med(ts["ease"]), ease_ms_min=round(float(np.min(ts["ease"])), 3),
                    itemknn_ms_median=med(ts["itemknn"]), itemknn_ms_min=round(float(np.min(ts["itemknn"])), 3),
                    ease_over_itemknn=round(float(np.median(ts["ease"]) / np.median(ts["itemknn"])), 3)))

    if not a.skip_large:
        xb = synthetic_big()
        with T.EASE(U, BIG_I, regularization=LAMBDA) as m:
            m.load(xb)
            ms = []
            for r in range(4):
                m.fit()
                if r >= 1:
                    ms.append(m.fit_ms_parts["inverse"])
            plan = T.ease.plan(BIG_I)
            emit(what="inverse", users=U, items=BIG_I, pairs=int(xb.nnz), regularization=LAMBDA, reps=3,
                 f64_bytes=plan["f64_bytes"], f32_bytes=plan["f32_bytes"], inverse_ms_median=med(ms),
                 inverse_ms_min=round(float(np.min(ms)), 3),
                 inverse_f64_tflops=round(float(BIG_I) ** 3 / (np.median(ms) * 1e-3) / 1e12, 3),
                 spec_sheet_f64_matrix_tflops=78.6)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
