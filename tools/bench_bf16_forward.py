"""Predict and evaluate from the bf16 snapshot against the float32 tables: one JSON object per shape.

Per shape the float32 entry and the bf16 entry alternate in one process on the same seeded ids (tables drawn on the device),
each launch between two device events on the model's stream: warm-up, then `--reps` launches each, median and minimum in us.
The forward shapes rotate through `--pool` id batches so that no launch finds its rows cached by the one before.  Bytes are
the algorithmic ones, computed here from the shape: two rows, 8 bytes of ids, 8 of biases and 4 of output (or of rate) per
rating; TB/s and the share of 8 TB/s follow from the median.  `--pnt-ab` adds, per forward shape, the bf16 launch with user
rows loaded non-temporally (TFR_BF16_PNT=1) and not (=0), alternating in the same loop.
python tools/bench_bf16_forward.py [--reps N] [--only name,...] [--pnt-ab] [--out profiles/bench_bf16_forward.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tfrecomm_amd as T
from tfrecomm_amd import bf16

HBM_TBS = 8.0

SHAPES = {
    # name: (U, I, D, B, item ids, entry)
    "ns_d128": (10_000_000, 1_000_000, 128, 262144, "uniform", "forward"),
    "ns_d64": (10_000_000, 1_000_000, 64, 262144, "uniform", "forward"),
    "ns_d128_zipf": (10_000_000, 1_000_000, 128, 262144, "zipf", "forward"),
    "ml1m_d64": (6040, 3706, 64, 10000, "uniform", "forward"),
    "eval_d128": (10_000_000, 1_000_000, 128, 1 << 20, "uniform", "eval"),
}


def bytes_per_launch(D, B):
    """(float32, bf16) algorithmic bytes of one launch of B ratings"""
    other = 8 + 8 + 4
    return B * (2 * D * 4 + other), B * (2 * bf16.row_stride(D) * 2 + other)


def draw_ids(rng, U, I, B, items):
    u = rng.integers(0, U, B).astype(np.int32)
    if items == "zipf":
        p = 1.0 / (np.arange(I, dtype=np.float64) + 50.0)
        i = rng.choice(I, B, p=p / p.sum()).astype(np.int32)
    else:
        i = rng.integers(0, I, B).astype(np.int32)
    return u, i


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def run_shape(name, reps, warmup, pool, pnt_ab, seed=0):
    U, I, D, B, items, entry = SHAPES[name]
    rng = np.random.default_rng(seed)
    stream = torch.cuda.Stream()
    m = T.SvdModel(U, I, D, optimizer="sgd")              # no Adam slots: the tables alone
    m.set_stream(stream.cuda_stream)
    m.init_tables(seed=seed + 1, feature_stddev=0.3, bias_stddev=0.5)
    m.snapshot_bf16()
    m.sync()
    arms = {}
    if entry == "forward":
        ids = [draw_ids(rng, U, I, B, items) for _ in range(pool)]
        dev = [(torch.from_numpy(u).cuda(), torch.from_numpy(i).cuda()) for u, i in ids]
        out = torch.empty(B, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        arms["f32"] = lambda k: m.forward_dev(dev[k][0].data_ptr(), dev[k][1].data_ptr(), B, out.data_ptr())
        bf = lambda k: m.forward_bf16_dev(dev[k][0].data_ptr(), dev[k][1].data_ptr(), B, out.data_ptr())
        arms["bf16"] = bf
        if pnt_ab:
            def forced(v):
                def go(k):
                    os.environ["TFR_BF16_PNT"] = v
                    try:
                        bf(k)
                    finally:
                        del os.environ["TFR_BF16_PNT"]
                return go
            arms["bf16_pnt1"], arms["bf16_pnt0"] = forced("1"), forced("0")
    else:
        pool = 1
        u, i = draw_ids(rng, U, I, B, items)
        r = rng.integers(1, 6, B).astype(np.float32)
        arms["f32"] = lambda k: m.eval(u, i, r)
        arms["bf16"] = lambda k: m.eval_bf16(u, i, r)
    ts = {a: [] for a in arms}
    for n in range(warmup + reps):
        for a, fn in arms.items():                        # the arms alternate, launch by launch, on the same id batch
            t = timed(stream, lambda: fn(n % pool))
            if n >= warmup:
                ts[a].append(t)
    m.sync()
    m.close()
    b32, b16 = bytes_per_launch(D, B)
    row = dict(shape=name, users=U, items=I, dim=D, batch=B, item_ids=items, entry=entry, reps=reps, id_batches=pool)
    for a, v in ts.items():
        nbytes = b32 if a == "f32" else b16
        med, best = float(np.median(v)), float(np.min(v))
        row[a] = dict(us_median=round(med, 2), us_min=round(best, 2), bytes=nbytes, tbs=round(nbytes / (med * 1e-6) / 1e12, 3),
                      frac_hbm=round(nbytes / (med * 1e-6) / 1e12 / HBM_TBS, 3))
    row["bf16_over_f32"] = round(row["bf16"]["us_median"] / row["f32"]["us_median"], 3)
    row["bf16_median_below_f32_min"] = bool(row["bf16"]["us_median"] < row["f32"]["us_min"])
    if entry == "eval":
        row["note"] = "host entry: the H2D copies of ids and rates (12 bytes per rating) and the read-back are inside both times"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pool", type=int, default=8, help="id batches a forward shape rotates through")
    ap.add_argument("--only", default="")
    ap.add_argument("--pnt-ab", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 50:
        print("note: fewer than 50 timed launches per entry", file=sys.stderr)
    torch.cuda.init()
    only = [s for s in a.only.split(",") if s]
    rows = []
    for name in SHAPES:
        if only and name not in only:
            continue
        rows.append(run_shape(name, a.reps, a.warmup, a.pool, a.pnt_ab))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
