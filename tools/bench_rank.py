"""Held-out ranking timings (tfr_rank_items): one JSON object per shape.

Per shape, on the same tables in the same process: the ranking call (`SvdModel.rank_items`, host entry, wall time per call
including staging and copies; median and best of `--reps`), `recommend_dev(k=10)` timed with device events, and a host
baseline - NumPy f32 ``P[users] @ Q.T`` + biases, then the counting of the contract per target (excluded items and NaN
dropped), timed on up to `--host-users` users and scaled linearly (labelled with the thread count and the users it ran on).
``frac_f32_matrix_peak_call`` divides the pairs' 2·D flops by the whole call's time; the counting kernel's own fraction
comes from a ``rocprofv3 --kernel-trace --stats`` run of this script.
``--bf16``: on the same shapes one model and one snapshot; `rank_items` and `rank_items_bf16` alternate call by call in one
process, 2 warm-up calls and `--reps` timed calls each, by the host clock around the whole call (staging and copies included;
median and minimum), and how far the two rankings differ on the held-out set.  No speed-up is promised: the counting does
the same integer work in both forms, only the tile gets cheaper.
python tools/bench_rank.py [--reps N] [--only name,...] [--bf16] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tfrecomm_amd as T

F32_MATRIX_PEAK_TF = 157.3      # MI355X f32-input MFMA peak


def tables(rng, U, I, D):
    return dict(mu=np.float32(0.1), bu=rng.standard_normal(U, dtype=np.float32) * .5,
                bi=rng.standard_normal(I, dtype=np.float32) * .5,
                P=rng.standard_normal((U, D), dtype=np.float32) * .3, Q=rng.standard_normal((I, D), dtype=np.float32) * .3)


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


def time_host(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts)), float(np.min(ts))


def host_baseline(t, users, tg, xp, xi, max_users):
    """NumPy on all cores: a block of users' score rows, then per target the eligible non-NaN items whose score beats it"""
    sub = min(users.size, max_users)
    I = t["Q"].shape[0]
    t0 = time.perf_counter()
    for b0 in range(0, sub, 64):
        u = users[b0:min(sub, b0 + 64)]
        s = t["P"][u] @ t["Q"].T
        s += t["mu"]
        s += t["bu"][u][:, None]
        s += t["bi"][None, :]
        for r in range(u.size):
            row = s[r]
            if xp is not None:
                row[xi[xp[b0 + r]:xp[b0 + r + 1]]] = -np.inf
            srt = np.sort(row[~np.isnan(row)])
            tt = tg[1][tg[0][b0 + r]:tg[0][b0 + r + 1]]
            I - np.searchsorted(srt, row[tt], side="right")
    dt = time.perf_counter() - t0
    return dict(host_us=round(dt * 1e6 * users.size / sub, 1), host_threads=os.cpu_count(), host_users_timed=int(sub))


def alternate_host(arms, reps, warmup=2):
    """arms: name -> call.  Warm-up and timed calls alternate the arms call by call."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    ts = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t0) * 1e6)
    return {name: (float(np.median(v)), float(np.min(v))) for name, v in ts.items()}


def run_bf16(name, t, users, tg, ex, reps):
    U, D = t["P"].shape
    I = t["Q"].shape[0]
    m = T.SvdModel(U, I, D)
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    m.snapshot_bf16()
    m.sync()
    res = alternate_host({"f32": lambda: m.rank_items(users, tg, exclude=ex),
                          "bf16": lambda: m.rank_items_bf16(users, tg, exclude=ex)}, reps)
    rf, rb = m.rank_items(users, tg, exclude=ex), m.rank_items_bf16(users, tg, exclude=ex)
    m.close()
    (fm, fb), (bm, bb) = res["f32"], res["bf16"]
    ranked = (rf >= 0) & (rb >= 0)
    d = np.abs(rf[ranked].astype(np.int64) - rb[ranked])
    return dict(shape=name, users=int(users.size), items=I, dim=D, targets=int(tg[1].size),
                exclusions=0 if ex is None else int(ex[1].size), reps=reps,
                f32_us_median=round(fm, 1), f32_us_min=round(fb, 1), bf16_us_median=round(bm, 1), bf16_us_min=round(bb, 1),
                bf16_over_f32=round(bm / fm, 3), same_rank_fraction=round(float(np.mean(d == 0)), 4),
                median_abs_rank_shift=float(np.median(d)), max_abs_rank_shift=int(d.max()),
                targets_in_top10_f32=round(float(np.mean((rf >= 0) & (rf < 10))), 5),
                targets_in_top10_bf16=round(float(np.mean((rb >= 0) & (rb < 10))), 5))


def run(name, t, users, tg, ex, reps, host_users, bf16=False):
    if bf16:
        return run_bf16(name, t, users, tg, ex, reps)
    U, D = t["P"].shape
    I = t["Q"].shape[0]
    m = T.SvdModel(U, I, D)
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    med, best = time_host(lambda: m.rank_items(users, tg, exclude=ex), reps)
    du = torch.from_numpy(users).cuda()
    dex = None if ex is None else (torch.from_numpy(ex[0]).cuda(), torch.from_numpy(ex[1]).cuda())
    rmed, rbest = time_dev(lambda: m.recommend_dev(du, 10, exclude=dex), reps)
    hmed, _ = time_host(lambda: m.recommend(users, 10, exclude=ex), max(3, reps // 2))
    m.sync()
    pairs = float(users.size) * I
    out = dict(shape=name, users=int(users.size), items=I, dim=D, targets=int(tg[1].size),
               exclusions=0 if ex is None else int(ex[1].size),
               rank_us_median=round(med, 1), rank_us_best=round(best, 1),
               recommend_dev_k10_us_median=round(rmed, 1), recommend_dev_k10_us_best=round(rbest, 1),
               recommend_host_k10_us_median=round(hmed, 1),
               rank_over_recommend_dev=round(med / rmed, 2),
               frac_f32_matrix_peak_call=round(2 * D * pairs / (med * 1e-6) / (F32_MATRIX_PEAK_TF * 1e12), 3))
    out.update(host_baseline(t, users, tg, None if ex is None else ex[0], None if ex is None else ex[1], host_users))
    m.close()
    return out


def ml1m(reps, host_users, bf16=False):
    rng = np.random.default_rng(0)
    U, I, D, N = 6040, 3706, 64, 1000209
    t = tables(rng, U, I, D)
    u, i = rng.integers(0, U, N), rng.integers(0, I, N)
    test = rng.random(N) < 0.2
    train_x = T.rated_matrix(u[~test], i[~test], U, I)
    tm = T.rated_matrix(u[test], i[test], U, I)
    users = np.flatnonzero(np.diff(tm.indptr)).astype(np.int32)
    tg = (np.ascontiguousarray(tm[users].indptr, np.int64), np.ascontiguousarray(tm[users].indices, np.int32))
    x = train_x[users]
    ex = (np.ascontiguousarray(x.indptr, np.int64), np.ascontiguousarray(x.indices, np.int32))
    return run("ml1m_80_20", t, users, tg, ex, reps, host_users, bf16)


def large(reps, host_users, bf16=False):
    rng = np.random.default_rng(1)
    U, I, D = 4096, 1 << 20, 64
    t = tables(rng, U, I, D)
    users = np.arange(U, dtype=np.int32)
    trows = [np.sort(rng.choice(I, 32, replace=False)) for _ in range(U)]
    xrows = [np.sort(rng.choice(I, 200, replace=False)) for _ in range(U)]
    tg = (np.arange(0, 32 * U + 1, 32, dtype=np.int64), np.concatenate(trows).astype(np.int32))
    ex = (np.arange(0, 200 * U + 1, 200, dtype=np.int64), np.concatenate(xrows).astype(np.int32))
    return run("large_4096x1M", t, users, tg, ex, reps, host_users, bf16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-users", type=int, default=128)
    ap.add_argument("--only", default="")
    ap.add_argument("--bf16", action="store_true", help="alternate rank_items and rank_items_bf16 on the same shapes")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.init()
    cases = {"ml1m_80_20": lambda: ml1m(a.reps, a.host_users, a.bf16),
             "large_4096x1M": lambda: large(a.reps, a.host_users, a.bf16)}
    only = [s for s in a.only.split(",") if s]
    lines = []
    for name, fn in cases.items():
        if only and name not in only:
            continue
        lines.append(json.dumps(fn()))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
