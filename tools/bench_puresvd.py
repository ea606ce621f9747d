"""PureSVD timings (tfr_psvd_*): one JSON object per measurement, on bench_itemknn.py's ML-1M-shaped synthetic pairs (6040
users x 3706 items, about 1 M distinct pairs, items drawn from a Zipf law, users uniform), factors = 64, oversample = 16,
8 iterations.

``fit``: the three device times tfr_psvd_fit reports (events around the products, the orthonormalisations, the eigen step
with the last products), medians and minima of ``--reps`` fits after 3 warm-up fits; ``residuals().max()`` after the fit;
beside them the wall time of ``scipy.sparse.linalg.svds(k=64)`` on the host (median of 3, at most 16 threads) and of the NumPy
restatement of the same algorithm (tests/puresvd_ref.py, once), for scale.
``product``: the product kernel alone at r = 80 columns in both orientations, device events around each launch
(tfr_psvd_product_ms), medians and minima; its algorithmic bytes per second count ``pairs * r * 8`` bytes read plus the rows
written.  Both dense blocks (2.4 MB and 3.9 MB) stay in the L2 / the Infinity Cache: the rate is one of cache requests, not
of HBM, and is not to be read against the HBM figure.
``recommend``: every user, k = 10, own items excluded, through ``to_svd_model()`` (wall clock around the host entry),
alternating call by call with ``ItemKNN.recommend`` (K = 20, cosine) in the same process.
``recommend_lists``: 256 lists (the first 256 users' rows as unknown users), k = 10, wall clock: fold-in, cast into the guest
rows and top-K.
These are records; no ratio is a gate.
python tools/bench_puresvd.py [--reps N] [--skip-host] [--out profiles/bench_puresvd.jsonl]"""
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
from tfrecomm_amd import puresvd
from tools.bench_itemknn import synthetic, wall, U, I

FACTORS, OVERSAMPLE, ITERATIONS = 64, 16, 8


def med(v):
    return round(float(np.median(v)), 3)


def low(v):
    return round(float(np.min(v)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.init()
    x = synthetic()
    nnz = int(x.nnz)
    plan = puresvd.plan(U, I, FACTORS, OVERSAMPLE)
    r = plan["r"]
    shape = dict(users=U, items=I, pairs=nnz, factors=FACTORS, oversample=OVERSAMPLE, iterations=ITERATIONS)
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    users = np.arange(U, dtype=np.int32)
    with T.PureSVD(U, I, FACTORS, OVERSAMPLE, ITERATIONS) as m, T.ItemKNN(U, I, K=20) as knn:
        m.load(x)
        parts = []
        for rep in range(3 + a.reps):
            m.fit()
            if rep >= 3:
                parts.append(m.fit_ms_parts)
        parts = np.array(parts)
        total = parts.sum(1)
        sigma = m.singular_values
        rec = dict(shape, what="fit", reps=a.reps, r=r, lanes=plan["lanes"], chunk=plan["chunk"], ahead=plan["ahead"],
                   fit_ms_median=med(total), fit_ms_min=low(total), products_ms_median=med(parts[:, 0]),
                   orthonormalise_ms_median=med(parts[:, 1]), eigen_and_factors_ms_median=med(parts[:, 2]), sweeps=m.sweeps(),
                   sigma_first=round(float(sigma[0]), 6), sigma_last=round(float(sigma[-1]), 6),
                   residual_max=float(m.residuals().max()))
        if not a.skip_host:
            from scipy.sparse.linalg import svds
            x64 = x.astype(np.float64)
            host = wall(lambda: svds(x64, k=FACTORS), 3, warmup=1)
            sv = np.sort(svds(x64, k=FACTORS, return_singular_vectors=False))[::-1]
            from tests import puresvd_ref as R
            t = time.perf_counter()
            ref = R.fit(np.ascontiguousarray(x.indptr, np.int64), np.ascontiguousarray(x.indices, np.int32), U, I, FACTORS, OVERSAMPLE,
                        ITERATIONS, m.start_block(0), plan["chunk"])
            rec.update(host_scipy_svds_ms_median=round(float(np.median(host)), 1), host_numpy_restatement_ms=round((time.perf_counter() - t) * 1e3, 1),
                       sigma_rel_to_svds_first=float(abs(sigma[0] / sv[0] - 1)), sigma_rel_to_svds_last=float(abs(sigma[-1] / sv[-1] - 1)),
                       sigma_max_rel_to_restatement=float(np.abs(sigma / ref["sigma"] - 1).max()))
        emit(**rec)

        for transpose, name, rows_out in ((False, "X V", U), (True, "X^T W", I)):
            m.product_ms(r, transpose, 3)
            ms = m.product_ms(r, transpose, max(a.reps, 10))
            moved = nnz * r * 8 + rows_out * r * 8
            emit(**dict(shape, what="product", product=name, r=r, reps=len(ms), ms_median=med(ms), ms_min=low(ms),
                        algorithmic_bytes=moved, algorithmic_gb_per_s_median=round(moved / (np.median(ms) * 1e-3) / 1e9, 1),
                        note="blocks of 2.4 MB and 3.9 MB stay in cache: a cache and request rate, not an HBM rate"))

        knn.fit(x)
        with m.to_svd_model(extra_users=256) as svd:
            arms = {"puresvd": lambda: svd.recommend(users, 10, exclude=x), "itemknn": lambda: knn.recommend(users, 10, exclude=x)}
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
                        puresvd_ms_median=med(ts["puresvd"]), puresvd_ms_min=low(ts["puresvd"]),
                        itemknn_ms_median=med(ts["itemknn"]), itemknn_ms_min=low(ts["itemknn"]),
                        puresvd_over_itemknn=round(float(np.median(ts["puresvd"]) / np.median(ts["itemknn"])), 3)))
            lists = x[:256]
            ms = wall(lambda: m.recommend_lists(svd, lists, 10), a.reps)
            emit(**dict(shape, what="recommend_lists", k=10, lists=256, reps=a.reps, ms_median=med(ms), ms_min=low(ms)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
