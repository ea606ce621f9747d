"""BPR step timings: one JSON line per shape, every leg at the same shape in the same process.

    python tools/bench_bpr.py [--shapes ml1m,ml10m] [--steps 100] [--out profiles/bench_bpr.jsonl]

Legs, at batch 10000, D 64, lazy Adam: the drawn BPR step (train_bpr_steps_drawn: pair draw, negative sampling and the step
on the device), the explicit host-fed step (train_bpr_step, negatives sampled on the device, one synchronising call per
step), the SVD model's drawn step (train_steps_drawn) on the same pairs as ratings, and a vectorised NumPy float32 host
restatement of one BPR step with host-sampled negatives (the CPU baseline; its thread count is reported).  Shapes are
synthetic: ML-1M-shaped (6040 x 3706, 1 M positives) and ML-10M-shaped (69878 x 10677, 10 M positives), item popularity
p(i) ~ 1 / (i + 50).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"ml1m": (6040, 3706, 1000209), "ml10m": (69878, 10677, 10000054)}


def pairs(U, I, n, seed=0):
    rs = np.random.RandomState(seed)
    w = 1.0 / (np.arange(I) + 50.0)
    u = rs.randint(0, U, n).astype(np.int32)
    i = rs.choice(I, n, p=w / w.sum()).astype(np.int32)
    return u, i


def host_step_f32(t, keys, u, i, rs, lam, alpha):
    """One BPR step in vectorised NumPy float32: uniform negatives, redrawn (up to 16 times) where they hit a positive, found
    by searchsorted in the sorted pair keys u * I + i; the scores, g, the scattered gradients and an SGD-shaped update."""
    P, Q, bi = t["P"], t["Q"], t["bi"]
    I = Q.shape[0]
    j = rs.randint(0, I, u.size)
    for _ in range(16):
        k = u.astype(np.int64) * I + j
        p = np.minimum(np.searchsorted(keys, k), keys.size - 1)
        hit = keys[p] == k
        if not hit.any():
            break
        j[hit] = rs.randint(0, I, int(hit.sum()))
    Pu, Qi, Qj = P[u], Q[i], Q[j]
    x = np.einsum("kd,kd->k", Pu, Qi - Qj) + bi[i] - bi[j]
    g = (-1.0 / (1.0 + np.exp(x))).astype(np.float32)
    dP = np.zeros_like(P)
    np.add.at(dP, u, g[:, None] * (Qi - Qj) + lam * Pu)
    dQ = np.zeros_like(Q)
    np.add.at(dQ, i, g[:, None] * Pu + lam * Qi)
    np.add.at(dQ, j, -g[:, None] * Pu + lam * Qj)
    dbi = np.zeros_like(bi)
    np.add.at(dbi, i, g)
    np.add.at(dbi, j, -g)
    P -= alpha * dP
    Q -= alpha * dQ
    bi -= alpha * dbi


def run_shape(name, steps, batch, dim, host_reps):
    import tfrecomm_amd as T
    U, I, n = SHAPES[name]
    u, i = pairs(U, I, n)
    X = T.rated_matrix(u, i, U, I)
    nnz = int(X.nnz)
    rowof = np.repeat(np.arange(U, dtype=np.int32), np.diff(X.indptr))
    row = dict(shape=name, users=U, items=I, positives=nnz, dim=dim, batch=batch, steps=steps)
    kw = dict(optimizer="adam", adam_mode="lazy", lr=1e-3, reg=0.005)
    with T.SvdModel(U, I, dim, **kw) as m:
        m.init_tables(seed=0, feature_stddev=0.1)
        m.set_positives(X)
        m.rng_seed(1)
        m.train_bpr_steps_drawn(batch, 5, want_loss=True)                  # warm-up: buffers and code objects
        t0 = time.perf_counter()
        loss = m.train_bpr_steps_drawn(batch, steps, want_loss=True)
        row["bpr_drawn_step_us"] = (time.perf_counter() - t0) / steps * 1e6
        row["bpr_mean_loss_last"] = float(loss[-1]) / batch
        rs = np.random.RandomState(2)
        hb = [rs.randint(0, nnz, batch) for _ in range(steps)]
        m.train_bpr_step(rowof[hb[0]], X.indices[hb[0]])
        t0 = time.perf_counter()
        skipped = 0
        for e in hb:
            skipped += m.train_bpr_step(rowof[e], X.indices[e])[3]
        row["bpr_explicit_step_us"] = (time.perf_counter() - t0) / steps * 1e6
        row["bpr_skipped_per_triple"] = skipped / float(steps * batch)
    with T.SvdModel(U, I, dim, **kw) as s:
        s.init_tables(seed=0)
        s.upload_triples(rowof, X.indices.astype(np.int32), np.ones(nnz, np.float32))
        s.rng_seed(1)
        s.train_steps_drawn(batch, 5, want_loss=True)
        t0 = time.perf_counter()
        s.train_steps_drawn(batch, steps, want_loss=True)
        row["svd_drawn_step_us"] = (time.perf_counter() - t0) / steps * 1e6
    rs2 = np.random.RandomState(3)
    t = dict(P=rs2.normal(0, .1, (U, dim)).astype(np.float32), Q=rs2.normal(0, .1, (I, dim)).astype(np.float32),
             bi=np.zeros(I, np.float32))
    it = np.asarray(X.indices, np.int32)
    keys = rowof.astype(np.int64) * I + it                                 # sorted: rows ascending, each row ascending
    t0 = time.perf_counter()
    for k in range(host_reps):
        e = hb[k % steps]
        host_step_f32(t, keys, rowof[e], it[e], rs2, np.float32(0.005), np.float32(1e-3))
    row["numpy_f32_step_us"] = (time.perf_counter() - t0) / host_reps * 1e6
    row["numpy_threads"] = int(os.environ.get("OMP_NUM_THREADS", "1"))
    row["bpr_drawn_over_svd_drawn"] = row["bpr_drawn_step_us"] / row["svd_drawn_step_us"]
    row["numpy_over_bpr_drawn"] = row["numpy_f32_step_us"] / row["bpr_drawn_step_us"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,ml10m")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    fh = open(a.out, "a") if a.out else None
    for name in a.shapes.split(","):
        row = run_shape(name, a.steps, a.batch, a.dim, a.host_reps)
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()})
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
