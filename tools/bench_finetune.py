"""Batched per-user fine-tuning (tfrecomm_amd.finetune's drivers with batched=True) against the sequential drivers.

Workloads (seeded, no data files):
  adaptive      ML-1M-shaped: 6040 users x 3952 items, D 20, nll, SGD lr 5e-3; every user 20 test items, budget 10,
                EPOCH_MAX 300, every user in one call
  non_adaptive  the same model, a ~100k-row test frame (1..32 rows per user, grouped by user), EPOCH_MAX 100
Per workload: the batched driver's wall time (warmed, the call synchronises the device; median and spread of --reps runs,
tables reset before each), the library call alone, the sequential driver on the first --sample users extrapolated to all of
them by rounds, the speed-up, row-steps per second (sum over rounds of prefix x EPOCH_MAX / call time) and the largest
|difference| of the predictions of the sampled users between the two paths.  --batched-only skips the sequential driver
(for a kernel-trace run).  One JSON line per workload on stdout; with --out, all of them in that file.

    python tools/bench_finetune.py [--reps 5] [--sample 50] [--batched-only] [--out bench_finetune.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfrecomm_amd as T                                   # noqa: E402
from tfrecomm_amd import finetune as FT                     # noqa: E402

U, I, D = 6040, 3952, 20


def tables(seed=0):
    rs = np.random.RandomState(seed)
    return dict(mu=np.float32(0.1), bu=rs.normal(0, .5, U).astype(np.float32), bi=rs.normal(0, .5, I).astype(np.float32),
                P=rs.normal(0, .1, (U, D)).astype(np.float32), Q=rs.normal(0, .1, (I, D)).astype(np.float32))


def frame(kind, seed=1):
    import pandas as pd
    rs = np.random.RandomState(seed)
    n = np.full(U, 20) if kind == "adaptive" else rs.randint(1, 33, U)
    u = np.repeat(np.arange(U), n)
    i = np.concatenate([rs.choice(I, k, replace=False) for k in n])
    r = (rs.rand(u.size) < 0.5).astype(np.float32)
    return pd.DataFrame(dict(user=u.astype(np.int32), item=i.astype(np.int32), outcome=r))


def model(t):
    m = T.SvdModel(U, I, D, loss="nll", optimizer="sgd", lr=5e-3, reg=0.05)
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    return m


def run(kind, m, df, E, batched, users=None):
    if kind == "adaptive":
        return FT.adaptive_test(m, df, budget=10, epoch_max=E, max_users=users, batched=batched)
    return FT.non_adaptive_test(m, df, epoch_max=E, max_user=users, batched=batched)


def preds(kind, res):
    if kind == "adaptive":
        return {r["user"]: np.asarray(r["predicted"], np.float64) for r in res}
    return np.asarray(res["pred"], np.float64)


def bench(kind, args):
    E = 300 if kind == "adaptive" else 100
    t, df = tables(), frame(kind)
    if kind == "adaptive":
        sched, _ = FT.adaptive_schedule(df, budget=10, epoch_max=E, max_users=None)
    else:
        sched, _ = FT.non_adaptive_schedule(df, epoch_max=E)
    row_steps = float(sched.prefix.astype(np.int64).sum()) * E
    m = model(t)
    run(kind, m, df, E, True)                               # warm: code objects, buffers
    wall, call = [], []
    for _ in range(args.reps):
        m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
        m.set_step(0, 0.9, 0.999)
        t0 = time.perf_counter()
        res = run(kind, m, df, E, True)
        wall.append(time.perf_counter() - t0)
    for _ in range(args.reps):
        m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
        t0 = time.perf_counter()
        m.finetune_users(sched.users, sched.row_ptr, sched.items, sched.rates, sched.round_ptr, sched.ask, sched.prefix,
                         E, round_seq=sched.seq)
        call.append(time.perf_counter() - t0)
    out = dict(workload=kind, users=int(sched.users.size), rounds=sched.n_rounds, rows=int(sched.row_ptr[-1]), epoch_max=E,
               row_steps=row_steps, batched_wall_s=dict(median=float(np.median(wall)), min=min(wall), max=max(wall)),
               call_s=dict(median=float(np.median(call)), min=min(call), max=max(call)),
               row_steps_per_s=row_steps / float(np.median(call)))
    if not args.batched_only:
        sample_users = args.sample
        if kind == "adaptive":
            seqm = model(t)
            t0 = time.perf_counter()
            want = run(kind, seqm, df[df["user"] < sample_users], E, False)   # the first users' rows only
            ts = time.perf_counter() - t0
            rounds_s = sum(len(r["asked"]) for r in want)
            got = preds(kind, res)
            dmax = max(float(np.abs(got[r["user"]] - np.asarray(r["predicted"])).max()) for r in want)
        else:
            seqm = model(t)
            last = int(sched.users[sample_users - 1])          # the frame is grouped by user, ids ascending
            t0 = time.perf_counter()
            want = run(kind, seqm, df, E, False, users=last)
            ts = time.perf_counter() - t0
            rounds_s = len(want["pred"])
            dmax = float(np.abs(preds(kind, res)[:rounds_s] - np.asarray(want["pred"])).max())
        seqm.close()
        extrap = ts * sched.n_rounds / rounds_s
        out.update(sequential_sample=dict(users=sample_users, rounds=rounds_s, wall_s=ts), sequential_extrapolated_s=extrap,
                   speedup=extrap / float(np.median(wall)), speedup_call=extrap / float(np.median(call)),
                   max_abs_pred_diff=dmax)
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=50)
    ap.add_argument("--batched-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for kind in ("adaptive", "non_adaptive"):
        r = bench(kind, args)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
