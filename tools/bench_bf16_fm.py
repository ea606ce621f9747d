"""The FM forward and FM top-K from the bf16 snapshot against the float32 tables: one JSON object per shape.

Forward shapes: BASELINE config 5 (1M features, D 64, 2^20 rows of 8 non-zeros, bench.py's draw) and a shape whose V fits
the Infinity Cache in either format (100k features).  Per shape one model and one snapshot; `forward_dev` and
`forward_bf16_dev` alternate launch by launch in one process on the same device CSR, the float32 launch twice per round
(arms f32 and f32_again) so that the float32 kernel's own spread is measured beside the difference.  Each launch is timed by
the handle's own event pair around the kernel (`FmModel.sync`): median and minimum in us.  Bytes are the algorithmic ones:
per non-zero one V row (4 D or 2 DP bytes) plus 12 bytes of index, value and weight, per row 8 bytes of row pointer and 4
of output (2156 and 1132 bytes per row at config 5); TB/s and the share of 8 TB/s follow from the median.
`--ntv-ab` adds the bf16 launch with non-temporal V loads forced on and off (TFR_FM_BF16_NTV=1 / 0) to the same loop.
An arm's time depends on what the launch before it left in the Infinity Cache, and the arms run in a fixed order: the
forced-on arm follows a float32 launch, the forced-off arm the forced-on one.  Repeated back to back the forced-on launch
is the slower one at config 5, so read the two forced arms as a check that the switch acts, not as the A/B.

Top-K shape: 4096 user features against a block of 2^20 item features, D 64, k 100: `topk` and `topk_bf16` alternate call by
call; both are host entries (ids in, items and scores out), timed by the host clock around the synchronous call.

python tools/bench_bf16_fm.py [--reps N] [--only name,...] [--ntv-ab] [--out profiles/bench_bf16_fm.jsonl]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tfrecomm_amd as T
from tfrecomm_amd import bf16

HBM_TBS = 8.0

FORWARD = {
    # name: (F, D, rows, nnz)
    "c5": (1_000_000, 64, 1 << 20, 8),
    "cached_d64": (100_000, 64, 1 << 20, 8),
}
TOPK = {"topk_4096_d64": (100_000, 1 << 20, 64, 4096, 100)}       # user features, item features, D, users, k


def bytes_per_row(D, nnz):
    """(float32, bf16) algorithmic bytes of one CSR row"""
    return nnz * (4 * D + 12) + 12, nnz * (2 * bf16.row_stride(D) + 12) + 12


def c5_rows(F, n, nnz, seed):
    """bench.py's draw scaled to F: one feature from the first 0.4 F, one from the next 0.2 F, nnz - 2 count-valued elsewhere"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    a, b = int(0.4 * F), int(0.6 * F)
    cols = [torch.randint(0, a, (n, 1), device="cuda", generator=g), torch.randint(a, b, (n, 1), device="cuda", generator=g),
            torch.randint(b, F, (n, nnz - 2), device="cuda", generator=g)]
    indices = torch.cat(cols, 1).to(torch.int32).contiguous()
    data = torch.cat([torch.ones(n, 2, device="cuda"), torch.randint(1, 4, (n, nnz - 2), device="cuda", generator=g).float()], 1).contiguous()
    indptr = (torch.arange(n + 1, device="cuda", dtype=torch.int64) * nnz).contiguous()
    return indptr, indices, data


def stats(us, nbytes=None):
    med, best = float(np.median(us)), float(np.min(us))
    out = dict(us_median=round(med, 2), us_min=round(best, 2), us_max=round(float(np.max(us)), 2))
    if nbytes is not None:
        out.update(bytes=nbytes, tbs=round(nbytes / (med * 1e-6) / 1e12, 3), frac_hbm=round(nbytes / (med * 1e-6) / 1e12 / HBM_TBS, 3))
    return out


def forced(call, value):
    def go():
        os.environ["TFR_FM_BF16_NTV"] = value
        try:
            call()
        finally:
            del os.environ["TFR_FM_BF16_NTV"]
    return go


def run_forward(name, reps, warmup, ntv_ab):
    F, D, n, nnz = FORWARD[name]
    indptr, indices, data = c5_rows(F, n, nnz, 13575)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    m = T.FmModel(F, D, loss="nll", optimizer="sgd", lr=1e-3, reg=1e-4)
    m.init(seed=3, stddev=0.1)
    m.snapshot_bf16()
    m.sync()
    args = (indptr.data_ptr(), indices.data_ptr(), data.data_ptr(), n, out.data_ptr())
    f32 = lambda: m.forward_dev(*args)
    b16 = lambda: m.forward_bf16_dev(*args)
    arms = {"f32": f32, "bf16": b16, "f32_again": f32}
    if ntv_ab:
        arms["bf16_ntv1"], arms["bf16_ntv0"] = forced(b16, "1"), forced(b16, "0")
    ts = {a: [] for a in arms}
    for k in range(warmup + reps):
        for a, fn in arms.items():
            fn()
            ms = m.sync()
            if k >= warmup:
                ts[a].append(ms * 1e3)
    m.close()
    b32, bb = bytes_per_row(D, nnz)
    row = dict(shape=name, features=F, dim=D, rows=n, nnz=nnz, reps=reps, bytes_per_row_f32=b32, bytes_per_row_bf16=bb,
               v_bytes_f32=F * D * 4, v_bytes_bf16=F * bf16.row_stride(D) * 2)
    for a, v in ts.items():
        row[a] = stats(v, n * (b32 if a.startswith("f32") else bb))
    f_med = [row["f32"]["us_median"], row["f32_again"]["us_median"]]
    row["f32_spread_us"] = round(max(row["f32"]["us_max"], row["f32_again"]["us_max"]) - min(row["f32"]["us_min"], row["f32_again"]["us_min"]), 2)
    row["f32_legs_differ_us"] = round(abs(f_med[0] - f_med[1]), 2)
    row["bf16_over_f32"] = round(row["bf16"]["us_median"] / min(f_med), 3)
    row["bf16_median_below_f32_min"] = bool(row["bf16"]["us_median"] < min(row["f32"]["us_min"], row["f32_again"]["us_min"]))
    return row


def run_topk(name, reps, warmup):
    Un, In, D, n, k = TOPK[name]
    F = Un + In
    m = T.FmModel(F, D)
    m.init(seed=5, stddev=0.3)
    m.snapshot_bf16()
    m.sync()
    users = np.random.default_rng(0).integers(0, Un, n).astype(np.int32)
    arms = {"f32": lambda: m.topk(users, Un, F, k), "bf16": lambda: m.topk_bf16(users, Un, F, k), "f32_again": lambda: m.topk(users, Un, F, k)}
    ts = {a: [] for a in arms}
    first = {}
    for r in range(warmup + reps):
        for a, fn in arms.items():
            t0 = time.perf_counter()
            items, _ = fn()
            dt = (time.perf_counter() - t0) * 1e6
            first[a] = items[:, 0]
            if r >= warmup:
                ts[a].append(dt)
    m.close()
    row = dict(shape=name, user_features=Un, item_features=In, dim=D, users=n, k=k, reps=reps,
               note="host entries: the copies of the ids in and of items and scores out are inside both times")
    for a, v in ts.items():
        row[a] = stats(v)
    row["bf16_over_f32"] = round(row["bf16"]["us_median"] / min(row["f32"]["us_median"], row["f32_again"]["us_median"]), 3)
    row["bf16_median_below_f32_min"] = bool(row["bf16"]["us_median"] < min(row["f32"]["us_min"], row["f32_again"]["us_min"]))
    row["top1_agreement"] = round(float(np.mean(first["f32"] == first["bf16"])), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--topk-reps", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--ntv-ab", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.init()
    only = [s for s in a.only.split(",") if s]
    rows = []
    for name in list(FORWARD) + list(TOPK):
        if only and name not in only:
            continue
        rows.append(run_forward(name, a.reps, a.warmup, a.ntv_ab) if name in FORWARD else run_topk(name, a.topk_reps, 2))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
