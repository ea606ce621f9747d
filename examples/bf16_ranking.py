"""What serving from the bf16 snapshot costs in ranking quality: `evaluate_ranking(m, ...)` on the float32 tables against
`evaluate_ranking(m, ..., bf16=True)` on the model's snapshot, on the same held-out set, and "more like this" from both.

The tables are SYNTHETIC: ML-1M-shaped (6040 users x 3706 items, dim 64) normal draws, the ones tools/bench_rank.py times,
with a random 80 / 20 split of 1M random (user, item) pairs.  They say how far rounding the rows to bf16 moves ranks at this
shape and scale of values; they say nothing about a trained model's absolute Recall or NDCG.  Load trained tables with
`m.set_tables(...)` (or train) to measure your own.

python examples/bf16_ranking.py [--dim D] [--ks 10,20]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import tfrecomm_amd as T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--ks", default="10,20")
    a = ap.parse_args()
    ks = tuple(int(k) for k in a.ks.split(","))
    rng = np.random.default_rng(0)
    U, I, D, N = 6040, 3706, a.dim, 1000209
    with T.SvdModel(U, I, D) as m:
        m.set_tables(np.float32(0.1), rng.standard_normal(U, dtype=np.float32) * .5, rng.standard_normal(I, dtype=np.float32) * .5,
                     rng.standard_normal((U, D), dtype=np.float32) * .3, rng.standard_normal((I, D), dtype=np.float32) * .3)
        u, i = rng.integers(0, U, N), rng.integers(0, I, N)
        test = rng.random(N) < 0.2
        train_x = T.rated_matrix(u[~test], i[~test], U, I)
        m.snapshot_bf16()
        f32 = T.evaluate_ranking(m, u[test], i[test], exclude=train_x, ks=ks)
        b16 = T.evaluate_ranking(m, u[test], i[test], exclude=train_x, ks=ks, bf16=True)
        print("synthetic ML-1M-shaped tables, dim %d: %d users, %d held-out items" % (D, f32["users"].size, f32["items"].size))
        print("%-12s %12s %12s %12s" % ("metric", "float32", "bf16", "bf16 - f32"))
        for k in ks:
            for name in ("recall@%d" % k, "ndcg@%d" % k):
                x, y = f32["mean"][name], b16["mean"][name]
                print("%-12s %12.6f %12.6f %+12.2e" % (name, x, y, y - x))
        for name in ("mrr", "auc"):
            x, y = f32["mean"][name], b16["mean"][name]
            print("%-12s %12.6f %12.6f %+12.2e" % (name, x, y, y - x))
        both = (f32["ranks"] >= 0) & (b16["ranks"] >= 0)
        shift = np.abs(f32["ranks"][both].astype(np.int64) - b16["ranks"][both])
        print("ranks: %.2f %% equal, median shift %g, largest %d of %d items" % (
            100 * np.mean(shift == 0), np.median(shift), shift.max(), I))
        items = np.arange(0, I, 37, dtype=np.int32)
        ni, _ = m.similar_items(items, 10)
        nb, _ = m.similar_items_bf16(items, 10)
        print("similar_items: nearest neighbour equal for %.1f %% of %d items, %.2f of 10 neighbours shared on average" % (
            100 * np.mean(ni[:, 0] == nb[:, 0]), items.size,
            np.mean([np.intersect1d(x, y).size for x, y in zip(ni, nb)])))


if __name__ == "__main__":
    main()
