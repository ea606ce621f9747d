"""Top-K from the bf16 snapshot against top-K from the float32 tables (tfr_bf16_topk_dev / tfr_topk_dev): one JSON object
per shape.

The shapes are those of tools/bench_topk.py.  Per shape one model, one snapshot, the same users and exclusions;
`recommend_dev` and `recommend_bf16_dev` alternate call by call in one process, 3 warm-up calls and `--reps` timed calls
each, timed with device events on the calling stream (median and minimum, us per call).  The snapshot's own cost
(`snapshot_bf16`: k_rows_to_bf16 on both tables and the bias copies, on the model's stream) is timed separately by the
host clock around the call and a `sync()`, and is in no timed call.
`cond` states the condition the shape is held to: on the large shapes the bf16 median below the float32 minimum; on the
latency-bound ones the bf16 median no more above the float32 median than the float32 arm's own median-to-minimum spread.
python tools/bench_bf16_topk.py [--reps N] [--only name,...]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tfrecomm_amd as T

BF16_MATRIX_PEAK_TF = 2516.6    # MI355X bf16 MFMA dense peak
F32_MATRIX_PEAK_TF = 157.3      # MI355X f32-input MFMA peak
WARMUP = 3


def tables(rng, U, I, D):
    return dict(mu=np.float32(0.1), bu=rng.standard_normal(U, dtype=np.float32) * .5,
                bi=rng.standard_normal(I, dtype=np.float32) * .5,
                P=rng.standard_normal((U, D), dtype=np.float32) * .3, Q=rng.standard_normal((I, D), dtype=np.float32) * .3)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternate(arms, reps):
    """arms: name -> call.  Warm-up and timed calls alternate the arms call by call."""
    for _ in range(WARMUP):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            ts[name].append(timed(fn))
    return {name: (float(np.median(v)), float(np.min(v))) for name, v in ts.items()}


def case(name, U, I, D, n, k, reps, large, excl=False, seed=0):
    rng = np.random.default_rng(seed)
    t = tables(rng, U, I, D)
    m = T.SvdModel(U, I, D)
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    users = np.arange(n, dtype=np.int32) if n == U else rng.integers(0, U, n).astype(np.int32)
    ex = None
    if excl:                                       # ML-1M-sized training set: 1M ratings
        X = T.rated_matrix(rng.integers(0, U, 1000209), rng.integers(0, I, 1000209), U, I)[users]
        ex = (torch.from_numpy(np.ascontiguousarray(X.indptr, np.int64)).cuda(),
              torch.from_numpy(np.ascontiguousarray(X.indices, np.int32)).cuda())
    du = torch.from_numpy(users).cuda()
    m.snapshot_bf16()
    m.sync()
    snap = []
    for _ in range(5):
        t0 = time.perf_counter()
        m.snapshot_bf16()
        m.sync()
        snap.append((time.perf_counter() - t0) * 1e6)
    res = alternate({"f32": lambda: m.recommend_dev(du, k, exclude=ex), "bf16": lambda: m.recommend_bf16_dev(du, k, exclude=ex)},
                    reps)
    m.sync()
    # the two arms answer the same question: the first place agrees but for near ties of the two number formats
    fi = m.recommend_dev(du[:64], k, return_scores=False)
    bi = m.recommend_bf16_dev(du[:64], k, return_scores=False)
    m.sync()
    agree = float((fi[:, 0] == bi[:, 0]).float().mean().item())
    m.close()
    (fm, fb), (bm, bb) = res["f32"], res["bf16"]
    pairs = float(n) * I
    out = dict(shape=name, users=n, items=I, dim=D, k=k, exclusions=bool(excl), reps=reps,
               f32_us_median=round(fm, 1), f32_us_min=round(fb, 1), bf16_us_median=round(bm, 1), bf16_us_min=round(bb, 1),
               bf16_over_f32=round(bm / fm, 3), snapshot_host_us_median=round(float(np.median(snap)), 1),
               f32_frac_f32_matrix_peak=round(2 * D * pairs / (fm * 1e-6) / (F32_MATRIX_PEAK_TF * 1e12), 3),
               bf16_frac_bf16_matrix_peak=round(2 * D * pairs / (bm * 1e-6) / (BF16_MATRIX_PEAK_TF * 1e12), 4),
               top1_agreement_first_64_users=round(agree, 3))
    if large:
        out["cond"] = "bf16 median < f32 min"
        out["cond_met"] = bool(bm < fb)
    else:
        out["cond"] = "bf16 median - f32 median <= f32 median - f32 min"
        out["cond_met"] = bool(bm - fm <= fm - fb)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    torch.cuda.init()
    cases = {
        "ml1m_all_users": lambda: case("ml1m_all_users", 6040, 3706, 64, 6040, 10, a.reps, False, excl=True),
        "large_d64": lambda: case("large_d64", 100000, 1 << 20, 64, 4096, 100, a.reps, True),
        "large_d128": lambda: case("large_d128", 100000, 1 << 20, 128, 4096, 100, a.reps, True),
        "one_user": lambda: case("one_user", 100000, 1 << 20, 64, 1, 50, a.reps, False),
    }
    only = [s for s in a.only.split(",") if s]
    for name, fn in cases.items():
        if only and name not in only:
            continue
        print(json.dumps(fn()), flush=True)


if __name__ == "__main__":
    main()
