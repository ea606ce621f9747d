"""Nearest-neighbour timings (tfr_neighbours_dev): one JSON object per shape and metric.

Per shape every item is a query (``similar_items_dev``, k = 10), timed with device events on the calling stream after warm-up
calls (median and best, us per call; the cosine form's first call builds the inverse norms and is a warm-up call, so the timed
calls are served from the cache).  Beside it, in the same process, ``recommend_dev`` for the same number of query rows over the
same number of candidates: a user table of item_num rows, so rows x candidates and the MFMA work are equal.  ``ratio`` =
neighbours / recommend_dev (medians).  ``rnorm_us``: the cosine form with the cache defeated (a table_devptr hand-out) minus
the cached form - what one k_row_rnorm pass costs.
``--bf16``: on the same shapes one model and one snapshot; ``similar_items_dev`` and ``similar_items_bf16_dev`` alternate call
by call in one process (3 warm-up calls, the first of which builds each form's inverse norms, and `--reps` timed calls each;
median and minimum), and the share of queries whose nearest neighbour is the same in both.
python tools/bench_neighbours.py [--reps N] [--only name,...] [--bf16] [--out profiles/bench_neighbours.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L

F32_MATRIX_PEAK_TF = 157.3      # MI355X f32-input MFMA peak


def time_dev(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def alternate(arms, reps, warmup=3):
    """arms: name -> call.  Warm-up and timed calls alternate the arms call by call."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b) * 1e3)
    return {name: (float(np.median(v)), float(np.min(v))) for name, v in ts.items()}


def case_bf16(name, I, D, k, reps, seed=0):
    rng = np.random.default_rng(seed)
    U = I
    m = T.SvdModel(U, I, D)
    m.set_tables(np.float32(0.1), rng.standard_normal(U, dtype=np.float32) * .5, rng.standard_normal(I, dtype=np.float32) * .5,
                 rng.standard_normal((U, D), dtype=np.float32) * .3, rng.standard_normal((I, D), dtype=np.float32) * .3)
    m.snapshot_bf16()
    m.sync()
    rows = torch.arange(I, dtype=torch.int32, device="cuda")
    out = []
    for metric in ("cosine", "dot"):
        res = alternate({"f32": lambda: m.similar_items_dev(rows, k, metric),
                         "bf16": lambda: m.similar_items_bf16_dev(rows, k, metric)}, reps)
        fi = m.similar_items_dev(rows, k, metric, return_scores=False)
        bi = m.similar_items_bf16_dev(rows, k, metric, return_scores=False)
        m.sync()
        (fm, fb), (bm, bb) = res["f32"], res["bf16"]
        out.append(dict(shape=name, metric=metric, rows=I, candidates=I, dim=D, k=k, reps=reps,
                        f32_us_median=round(fm, 1), f32_us_min=round(fb, 1), bf16_us_median=round(bm, 1),
                        bf16_us_min=round(bb, 1), bf16_over_f32=round(bm / fm, 3),
                        top1_agreement=round(float((fi[:, 0] == bi[:, 0]).float().mean().item()), 4)))
    m.close()
    return out


def case(name, I, D, k, reps, seed=0, bf16=False):
    if bf16:
        return case_bf16(name, I, D, k, reps, seed)
    rng = np.random.default_rng(seed)
    U = I                                           # recommend_dev over the same rows x candidates
    m = T.SvdModel(U, I, D)
    m.set_tables(np.float32(0.1), rng.standard_normal(U, dtype=np.float32) * .5, rng.standard_normal(I, dtype=np.float32) * .5,
                 rng.standard_normal((U, D), dtype=np.float32) * .3, rng.standard_normal((I, D), dtype=np.float32) * .3)
    rows = torch.arange(I, dtype=torch.int32, device="cuda")
    rec_med, rec_best = time_dev(lambda: m.recommend_dev(rows, k), reps)
    out = []
    for metric in ("cosine", "dot"):
        med, best = time_dev(lambda: m.similar_items_dev(rows, k, metric), reps)
        pairs = float(I) * I
        out.append(dict(shape=name, metric=metric, rows=I, candidates=I, dim=D, k=k, us_median=round(med, 1),
                        us_best=round(best, 1), recommend_dev_us_median=round(rec_med, 1),
                        recommend_dev_us_best=round(rec_best, 1), ratio=round(med / rec_med, 3),
                        frac_f32_matrix_peak=round(2 * D * pairs / (med * 1e-6) / (F32_MATRIX_PEAK_TF * 1e12), 3)))
    m.sync()
    m.table_devptr(L.Q)                             # from here on every cosine query rebuilds the inverse norms
    med, _ = time_dev(lambda: m.similar_items_dev(rows, k, "cosine"), reps)
    out[0]["rnorm_us"] = round(med - out[0]["us_median"], 1)
    m.sync()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--bf16", action="store_true", help="alternate similar_items_dev and similar_items_bf16_dev")
    a = ap.parse_args()
    torch.cuda.init()
    cases = {
        "ml1m_all_items": lambda: case("ml1m_all_items", 3706, 64, 10, a.reps, bf16=a.bf16),
        "ml10m_all_items": lambda: case("ml10m_all_items", 10677, 64, 10, a.reps, bf16=a.bf16),
    }
    only = [s for s in a.only.split(",") if s]
    lines = []
    for name, fn in cases.items():
        if only and name not in only:
            continue
        for rec in fn():
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
